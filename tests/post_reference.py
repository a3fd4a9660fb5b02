"""The detection post-processing rule and the adversarial inputs it is tested on (no GPU): si_hip_yolo_postprocess_f32
(simpleinfer_amd/csrc/hip/postprocess.hip) against test/test_yolo/test_yolo.cpp:337-428, restated here in numpy fp32.

THE RULE.  Per image: confidence = box score * first maximum class score (strict '>', starting from -FLT_MAX, so a row whose class scores are
all -inf, all NaN or all -FLT_MAX has label -1 and class score -FLT_MAX); kept when confidence >= prob_threshold; sorted by confidence,
descending; greedy NMS against every box PICKED so far (same label only unless agnostic), suppressed when inter / union > nms_threshold
(strict); un-letterbox + clip when `adjust` is given.  Every comparison is an explicit select (`a > b ? a : b` is np.where(a > b, a, b)):
Python's max / min, np.maximum / np.fmax and np.clip differ from one when an operand is NaN or when +0 meets -0.  Two kinds occur.  The clip is
the reference's own text, std::max(lo, std::min(v, hi)) (test_yolo.cpp:188-191): std::min(a, b) is `b < a ? b : a`, std::max(a, b) is
`a < b ? b : a`, the FIRST argument when the compare is false, so NaN clips to lo and -0.0 to +0.0.  The box intersection is simpleocv's
`a & b`, which is NOT in the reference checkout: its min / max are taken as the oracle takes them (oracle/si_oracle.c), `a > b ? a : b` and
`a < b ? a : b` with the candidate first -- an assumption of the oracle's, which this rule and the kernel are held to.

The sort follows the DEVICE's documented tie rule (include/si_hip.h), not the reference's unstable quicksort: equal-comparing confidences stay
in element order.  ONE EXCEPTION: the device keys on the BITS of the confidence, so a +0 confidence sorts ahead of a -0 one whatever their
element order (the two compare equal).  Both can only survive a prob_threshold <= 0.  `sort_order` restates that through the same
order-preserving map of the bits.

THE CASES.  `cases()` is the table: every generator returns pred [n][rows][ne] with a different variant per image, its thresholds, an
`adjust` and the structural facts it promises (tests/test_postprocess_cpu.py asserts them from this rule alone, so a generator that misses its
boundary fails there and not silently on the GPU).  chain: the in-chunk dependency chain of the two NMS kernels; counts: the 64 / 128 / 256 /
1024 boundaries of the filter, the rank sort, the chunk walk, the four-wave split and the compaction; bins: the segment prefix at 64 / 65 / 66
bins and the LDS limit ne = 128; classes: label -1, tied maxima, NaN and +inf confidences; equalities: confidence == threshold, IoU ==
threshold and one ulp either side; geometry: zero-area, negative and non-finite boxes, clip under a tiny and a huge scale; ties: equal
confidences that overlap, and +0 against -0."""
import functools
from typing import NamedTuple

import numpy as np

F = np.float32
FLT_MAX = np.finfo(np.float32).max
PROB_THR, NMS_THR = F(0.25), F(0.45)


# ---- the rule -----------------------------------------------------------------------------------------------------------------------------
def sel_gt(a, b):
    """a > b ? a : b"""
    return np.where(a > b, a, b)


def sel_lt(a, b):
    """a < b ? a : b"""
    return np.where(a < b, a, b)


def ordered_bits(conf):
    """the order-preserving map float -> u32 the device sorts on (larger float <=> larger integer; +0 above -0)"""
    u = np.ascontiguousarray(conf, F).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def filter_rows(pred, prob_threshold):
    """test_yolo.cpp:341-377 on pred [rows][ne] -> (element index, box [k][4] = x, y, w, h, label, confidence) of the survivors, element order"""
    p = np.ascontiguousarray(pred, F)
    rows, ne = p.shape
    score = np.full(rows, -FLT_MAX, F)
    label = np.full(rows, -1, np.int32)
    for k in range(ne - 5):
        s = p[:, 5 + k]
        up = s > score
        label[up] = k
        score[up] = s[up]
    conf = p[:, 4] * score
    keep = np.nonzero(conf >= F(prob_threshold))[0]
    cx, cy, w, h = (p[keep, i] for i in range(4))
    x0, y0 = cx - w * F(0.5), cy - h * F(0.5)
    x1, y1 = cx + w * F(0.5), cy + h * F(0.5)
    return keep, np.stack([x0, y0, x1 - x0, y1 - y0], 1).astype(F), label[keep], conf[keep]


def sort_order(elem, conf):
    """descending confidence, equal-comparing confidences in element order -- on the bits, so +0 goes ahead of -0"""
    return np.lexsort((elem, -ordered_bits(conf).astype(np.int64)))


def nms(box, label, nms_threshold, agnostic):
    """test_yolo.cpp:68-104 over candidates in sorted order -> indices picked.  The inner loop over the picked list is one vector expression."""
    n = len(box)
    thr = F(nms_threshold)
    x, y = box[:, 0], box[:, 1]
    x2, y2 = box[:, 0] + box[:, 2], box[:, 1] + box[:, 3]
    area = box[:, 2] * box[:, 3]
    picked = np.empty(n, np.int64)
    P = 0
    for i in range(n):
        if P:
            j = picked[:P]
            ix = sel_gt(x[i], x[j])
            iy = sel_gt(y[i], y[j])
            w = sel_lt(x2[i], x2[j]) - ix
            h = sel_lt(y2[i], y2[j]) - iy
            ia = np.where((w <= 0) | (h <= 0), F(0), w * h)
            ua = area[i] + area[j] - ia
            s = ia / ua > thr
            if not agnostic:
                s &= label[j] == label[i]
            if s.any():
                continue
        picked[P] = i
        P += 1
    return picked[:P].copy()


def clip(v, lo, hi):
    """test_yolo.cpp:188-191, std::max(lo, std::min(v, hi)): m = hi < v ? hi : v; lo < m ? m : lo"""
    m = np.where(hi < v, hi, v)
    return np.where(lo < m, m, lo)


def finish(box, label, conf, adjust):
    """test_yolo.cpp:386-416: rows {x, y, w, h, confidence, label}, un-letterboxed and clipped when adjust = {pad_l, pad_t, scale, cols, rows}"""
    d = np.zeros((len(box), 6), F)
    if adjust is None:
        d[:, :4] = box
    else:
        pl, pt, sc, cols, rows = (F(v) for v in adjust)
        xmax, ymax = cols - F(1), rows - F(1)
        x0 = clip((box[:, 0] - pl) / sc, F(0), xmax)
        y0 = clip((box[:, 1] - pt) / sc, F(0), ymax)
        x1 = clip(((box[:, 0] + box[:, 2]) - pl) / sc, F(0), xmax)
        y1 = clip(((box[:, 1] + box[:, 3]) - pt) / sc, F(0), ymax)
        d[:, 0], d[:, 1], d[:, 2], d[:, 3] = x0, y0, x1 - x0, y1 - y0
    d[:, 4] = conf
    d[:, 5] = label.astype(F)
    return d


def postprocess_image(pred, prob_threshold, nms_threshold, agnostic=False, adjust=None):
    """one image: pred [rows][ne] -> dets [picks][6] in picked order (no cap: the entry's max_det only cuts this list)"""
    with np.errstate(all="ignore"):
        elem, box, label, conf = filter_rows(pred, prob_threshold)
        o = sort_order(elem, conf)
        box, label, conf = box[o], label[o], conf[o]
        p = nms(box, label, nms_threshold, agnostic)
        return finish(box[p], label[p], conf[p], adjust)


def postprocess(pred, prob_threshold, nms_threshold, agnostic=False, adjust=None):
    """pred [n][rows][ne] -> (list of dets per image, counts int32 [n]), the shape of hipops.yolo_postprocess's result"""
    outs = [postprocess_image(pred[b], prob_threshold, nms_threshold, agnostic, None if adjust is None else adjust[b])
            for b in range(len(pred))]
    return outs, np.asarray([len(d) for d in outs], np.int32)


def survivors(pred, prob_threshold):
    """per image: (labels, confidences) of the rows the filter keeps, sorted"""
    out = []
    for b in range(len(pred)):
        with np.errstate(all="ignore"):
            elem, _, label, conf = filter_rows(pred[b], prob_threshold)
        o = sort_order(elem, conf)
        out.append((label[o], conf[o]))
    return out


def assert_same(got, ref, what=""):
    """assert_exact that also holds on non-finite boxes and on the sign of zero: the same shape, NaN in the same places (a NaN's sign and
    payload are the producing machine's, not the rule's) and the same BITS everywhere else"""
    got, ref = np.ascontiguousarray(got, F), np.ascontiguousarray(ref, F)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    gn, rn = np.isnan(got), np.isnan(ref)
    assert np.array_equal(gn, rn), "%s: NaN in %d places, expected in %d; first difference at %s" % (
        what, int(gn.sum()), int(rn.sum()), tuple(np.argwhere(gn != rn)[0]))
    bad = (got.view(np.uint32) != ref.view(np.uint32)) & ~rn
    assert not bad.any(), "%s: %d of %d elements differ in bits, first at %s: got %r, expected %r" % (
        what, int(bad.sum()), ref.size, tuple(np.argwhere(bad)[0]), got[bad][0], ref[bad][0])


def assert_same_result(got, ref, what=""):
    (gd, gc), (rd, rc) = got, ref
    assert list(gc) == list(rc), "%s: counts %s, expected %s" % (what, list(gc), list(rc))
    for b, (g, r) in enumerate(zip(gd, rd)):
        assert_same(g, r, "%s image %d" % (what, b))


# ---- building blocks of the generators ----------------------------------------------------------------------------------------------------
def _rng(seed):
    return np.random.Generator(np.random.Philox(seed))


def _rows(boxes, conf, label, nc, r):
    """prediction rows for boxes [k][4] = x, y, w, h: class score 1.0 at `label`, below 0.5 elsewhere, so the confidence is exactly `conf`"""
    boxes = np.asarray(boxes, np.float64).reshape(-1, 4)
    k = len(boxes)
    p = np.empty((k, 5 + nc), F)
    p[:, 0] = boxes[:, 0] + boxes[:, 2] * 0.5
    p[:, 1] = boxes[:, 1] + boxes[:, 3] * 0.5
    p[:, 2:4] = boxes[:, 2:4]
    p[:, 4] = np.asarray(conf, F)
    p[:, 5:] = r.uniform(0.0, 0.5, (k, nc))
    p[np.arange(k), 5 + np.asarray(label, np.int64)] = 1.0
    return p


def _cold(rows, nc, r, sign=1.0):
    """rows the filter drops: confidence in (0, 0.05) (sign = -1: negative, for thresholds <= 0)"""
    p = np.empty((rows, 5 + nc), F)
    p[:, 0:2] = r.uniform(0, 640, (rows, 2))
    p[:, 2:4] = r.uniform(4, 300, (rows, 2))
    p[:, 4] = sign * r.uniform(0.01, 0.1, rows)
    p[:, 5:] = r.uniform(0.05, 0.5, (rows, nc))
    return p


def _embed(surv, rows, r, keep_order=False, sign=1.0):
    """the survivors scattered among `rows` - len(surv) dropped rows: at random positions, in random order unless keep_order"""
    nc = surv.shape[1] - 5
    assert len(surv) <= rows
    out = _cold(rows, nc, r, sign)
    pos = np.sort(r.choice(rows, len(surv), replace=False))
    if not keep_order:
        pos = r.permutation(pos)
    out[pos] = surv
    return out


def _ladder(k, r=None, base=0.3, step=2.0 ** -13):
    """k distinct confidences above the default threshold, descending -- shuffled when an rng is given"""
    c = (base + step * np.arange(k, 0, -1)).astype(F)
    assert len(np.unique(c)) == k and c.min() > PROB_THR and c.max() < 1
    return c if r is None else r.permutation(c)


def _odd_rows(rows):
    """never a multiple of the filter's 128 rows per block"""
    return rows + 1 if rows % 128 == 0 else rows


def _adjust(n):
    return np.asarray([[8 + 3 * b, 5 + 2 * b, 0.5 + 0.25 * b, 640, 480] for b in range(n)], F)


class Case(NamedTuple):
    id: str
    pred: np.ndarray        # [n][rows][ne]
    prob_thr: np.float32
    nms_thr: np.float32
    adjust: np.ndarray      # [n][5]
    distinct: bool          # no two survivors of an image compare equal: the reference's unstable quicksort has one answer
    facts: dict


def _case(cid, images, facts, prob_thr=PROB_THR, nms_thr=NMS_THR, adjust=None, distinct=True):
    pred = np.ascontiguousarray(np.stack(images), F)
    return Case(cid, pred, F(prob_thr), F(nms_thr), _adjust(len(pred)) if adjust is None else np.asarray(adjust, F), distinct, facts)


# ---- chain ----------------------------------------------------------------------------------------------------------------------------------
def chain(length, interleaved=False):
    """`length` 10x10 boxes on one row, 3 apart (neighbour IoU 7/13 > 0.45, next-but-one 4/16 < 0.45), confidence falling along the row: the
    greedy answer is every second box, and 'suppressed by any earlier candidate' would keep the first alone.  Image p puts p isolated boxes in
    front, so that the chain box at sorted position 63 (lane 63 of the first chunk) is alive for p = 1, 3 and dead for p = 0, 2, and whether
    position 64 (lane 0 of the next chunk) lives is decided across the chunk boundary.  interleaved: a second label's chain, one pixel to the
    right, alternating with the first in confidence -- per class the two must not interact, agnostic they must."""
    nc = 2
    images = []
    for phase in range(4):
        r = _rng(1000 + length * 8 + phase + (4 if interleaved else 0))
        k = np.arange(length)
        boxes_a = np.stack([3.0 * k, 0 * k, 10 + 0 * k, 10 + 0 * k], 1)
        iso = np.stack([40.0 * np.arange(phase), 1000 + 0.0 * np.arange(phase), 10 + 0.0 * np.arange(phase), 10 + 0.0 * np.arange(phase)], 1)
        if interleaved:
            boxes_b = boxes_a + np.asarray([1.0, 0, 0, 0])
            boxes = np.concatenate([iso, np.stack([boxes_a, boxes_b], 1).reshape(-1, 4)])
            label = np.concatenate([np.zeros(phase, np.int64), np.tile([0, 1], length)])
        else:
            boxes = np.concatenate([iso, boxes_a])
            label = np.zeros(len(boxes), np.int64)
        conf = (1.0 - np.arange(len(boxes)) * 2.0 ** -12).astype(F)      # exact in fp32, falling with the sorted position
        images.append(_embed(_rows(boxes, conf, label, nc, r), _odd_rows(len(boxes) - phase + 153), r))
    return _case("chain%s_%d" % ("2" if interleaved else "", length), images, {"length": length, "interleaved": interleaved})


# ---- counts ---------------------------------------------------------------------------------------------------------------------------------
COUNTS = (1, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1023, 1024, 1025, 2049)
LAYOUTS = ("far", "identical", "dense")


def counts(count, nc=3):
    """exactly `count` candidates per image, distinct confidences, scattered among dropped rows; image 0: all far apart (everything is picked,
    so the picked list has the candidate list's length), image 1: all identical (one pick), image 2: random dense (real chains)"""
    rows = _odd_rows(count + count // 8 + 37)
    images = []
    for li, layout in enumerate(LAYOUTS):
        r = _rng(2000 + count * 4 + li + 16 * nc)
        if layout == "far":
            k = np.arange(count)
            boxes = np.stack([20.0 * (k % 50), 20.0 * (k // 50), 10 + 0.0 * k, 10 + 0.0 * k], 1)
            label = r.integers(0, nc, count)
        elif layout == "identical":
            boxes = np.tile([100.0, 120.0, 30.0, 40.0], (count, 1))
            label = np.full(count, nc // 2)
        else:
            boxes = np.concatenate([r.uniform(0, 200, (count, 2)), r.uniform(20, 80, (count, 2))], 1)
            label = r.integers(0, nc, count)
        images.append(_embed(_rows(boxes, _ladder(count, r), label, nc, r), rows, r))
    return _case("counts_%d%s" % (count, "" if nc == 3 else "_nc%d" % nc), images, {"count": count, "nc": nc})


# ---- bins -----------------------------------------------------------------------------------------------------------------------------------
BINS_NC = (1, 3, 63, 64, 65, 80, 123)


def bins(nc):
    """nc classes (nc + 1 bins; ne = 128 at nc = 123 is the filter's LDS limit): some labels empty, the last label never, and one label with
    more than 64 far-apart candidates -- the label in the middle in image 0, the LAST one in image 1, behind the longest prefix, where image 1
    also holds a label -1 row that shifts every segment by one"""
    images, facts = [], {"nc": nc, "heavy": []}
    for b in range(2):
        r = _rng(3000 + nc * 2 + b)
        heavy = (nc // 2, nc - 1)[b]
        empty = {k for k in range(nc - 1) if k != heavy and (k == 0 or k % 5 == 3)}
        k = np.arange(70)
        boxes = [np.stack([20.0 * (k % 35), 300 + 20.0 * (k // 35), 10 + 0.0 * k, 10 + 0.0 * k], 1),        # 70 far apart: 70 picks
                 np.concatenate([r.uniform(400, 440, (12, 2)), r.uniform(30, 60, (12, 2))], 1)]               # 12 that overlap
        label = [np.full(82, heavy)]
        for lab in range(nc):
            if lab == heavy or lab in empty:
                continue
            m = int(r.integers(1, 4))
            boxes.append(np.concatenate([r.uniform(0, 200, (m, 2)), r.uniform(20, 80, (m, 2))], 1))
            label.append(np.full(m, lab))
        boxes, label = np.concatenate(boxes), np.concatenate(label)
        surv = _rows(boxes, _ladder(len(boxes), r), label, nc, r)
        if b == 1:
            none = _rows([[500, 20, 30, 30]], [-1.0], [0], nc, r)
            none[:, 5:] = -np.inf                                                                             # confidence FLT_MAX, label -1
            surv = np.concatenate([surv, none])
        images.append(surv)
        facts["heavy"].append(heavy)
    rows = _odd_rows(max(len(s) for s in images) + 41)
    return _case("bins_%d" % nc, [_embed(s, rows, _rng(3500 + nc + b)) for b, s in enumerate(images)], facts)


# ---- classes --------------------------------------------------------------------------------------------------------------------------------
def classes():
    """what the class scan and the filter do at their edges (nc = 4): tied maxima (the first wins), no maximum at all (label -1: every score
    -inf, NaN or exactly -FLT_MAX; kept when the box score is negative), NaN confidences (dropped), one +inf confidence (first)"""
    nc = 4
    inf, nan = np.inf, np.nan
    # (box score, class scores, box, expected label or None when the row is dropped)
    table = [
        (0.9, [0.5, 0.9, 0.9, 0.3], (50, 50, 20, 20), 1),
        (0.8, [0.9, 0.9, 0.9, 0.9], (90, 50, 20, 20), 0),
        (-1.0, [-inf] * 4, (300, 300, 20, 20), -1),                      # confidence FLT_MAX
        (-2.0 ** -126, [nan] * 4, (300, 300, 20, 20), -1),               # confidence 4 - 2^-22, suppressed by the row above (same label -1)
        (-0.5, [-inf] * 4, (400, 300, 20, 20), -1),
        (inf, [0.1, 0.2, 0.3, 0.4], (130, 50, 20, 20), 3),               # +inf: first
        (nan, [0.1, 0.9, 0.3, 0.4], (170, 50, 20, 20), None),
        (0.0, [inf, 0.2, 0.3, 0.4], (210, 50, 20, 20), None),            # 0 * inf
        (0.7, [nan, 0.7, nan, 0.2], (250, 50, 20, 20), 1),
        (0.6, [-FLT_MAX] * 4, (290, 50, 20, 20), None),                  # not > -FLT_MAX: label -1, confidence negative
        (-2.0 ** -10, [-FLT_MAX] * 4, (330, 50, 20, 20), -1),
        (0.5, [0.2, 0.6, -inf, 0.6], (370, 50, 20, 20), 1),
    ]
    images = []
    for b in range(2):
        r = _rng(4000 + b)
        special = np.empty((len(table), 5 + nc), F)
        for i, (bs, cs, (x, y, w, h), _) in enumerate(table):
            special[i] = [x + w * 0.5, y + h * 0.5, w, h, bs] + cs
        m = 40
        back = _rows(np.concatenate([r.uniform(0, 200, (m, 2)) + 100, r.uniform(20, 80, (m, 2))], 1), _ladder(m, r), r.integers(0, nc, m), nc, r)
        surv = np.concatenate([special, back] if b == 0 else [back, special[::-1]])
        images.append(_embed(surv, 101, r))
    want = sorted(t[3] for t in table if t[3] is not None)
    return _case("classes", images, {"special_labels": want, "dropped": sum(t[3] is None for t in table), "background": 40})


# ---- equalities -----------------------------------------------------------------------------------------------------------------------------
IOU_EQ = F(8) / F(24)      # boxes (0, 0, 4, 4) and (2, 0, 4, 4): intersection 8, union 24, and the fp32 quotient is this number


def equalities():
    """[iou_eq, iou_below, conf_eq]: an IoU EQUAL to nms_threshold does not suppress (strict '>') and one ulp less of threshold does -- which
    also needs the device's division to be the correctly rounded one; a confidence EQUAL to prob_threshold is kept ('>='), one ulp below is not"""
    nc = 1
    out = []
    for cid, thr in (("iou_eq", IOU_EQ), ("iou_below", np.nextafter(IOU_EQ, F(0)))):
        r = _rng(5000)
        surv = _rows([[0, 0, 4, 4], [2, 0, 4, 4]], [0.9, 0.8], [0, 0], nc, r)
        out.append(_case("equalities_" + cid, [_embed(surv, 9, r)], {"picks": 2 if cid == "iou_eq" else 1}, nms_thr=thr))
    thr = F(0.3)
    r = _rng(5001)
    surv = _rows([[0, 0, 10, 10], [40, 0, 10, 10], [80, 0, 10, 10]], [thr, np.nextafter(thr, F(0)), np.nextafter(thr, F(1))], [0, 0, 0], nc, r)
    out.append(_case("equalities_conf_eq", [_embed(surv, 9, r)], {"picks": 2, "lowest": thr}, prob_thr=thr))
    return out


# ---- geometry -------------------------------------------------------------------------------------------------------------------------------
def geometry(nms_thr=NMS_THR, cid="geometry"):
    """degenerate and non-finite boxes among ordinary ones, distinct confidences.  The special rows all carry label 0 and sit at the TOP of
    the confidence order in images 0 and 3 (they are picked first: the odd value is on the picked side of every later comparison), at the
    BOTTOM in image 1 (the candidate side) and anywhere in image 2.  adjust: an ordinary letterbox, a tiny scale (everything clips to the far
    edge), a huge one (everything collapses to 0, and a slightly negative x becomes -0.0, which the reference's std::max(0, .) turns into +0.0;
    NaN coordinates clip to 0 by the same rule), an ordinary one.  With a negative nms_threshold (geometry_negthr) IoU 0 suppresses too, which is where the intersection's
    min / max form matters: see test_postprocess_cpu.py."""
    nc = 2
    inf, nan = np.inf, np.nan
    special = []
    for f in range(4):                                           # NaN, +inf, -inf in each box field; first, so that image 0 picks them first
        for v in (nan, inf, -inf):
            row = [220.0, 220.0, 40.0, 40.0]
            row[f] = v
            special.append(tuple(row))
    special += [
        (50, 50, 0, 0), (50, 50, 0, 0),                          # zero-area duplicates: 0 / 0
        (60, 55, 0, 10), (60, 55, 0, 10),                        # zero width
        (110, 115, -20, 30), (110, 115, 20, -30), (100, 105, -20, -30), (110, 110, 30, 30),      # negative w, h, both (positive area), a plain box over them
        (-475, -375, 50, 50), (5050, 4050, 100, 100),            # wholly outside the image
        (0.25 - 2.0 ** -26, 300.25, 0.5, 0.5),                   # x0 = -2^-26: -0.0 after the huge scale, +0.0 after the clip
        (225, 225, 40, 40), (215, 215, 40, 40),                  # plain boxes over the non-finite ones
    ]
    special = np.asarray(special, F)        # (cx, cy, w, h) as the prediction holds them
    ns, nb = len(special), 60
    adjust = [[10, 20, 0.5, 640, 480], [10, 20, 1e-30, 640, 480], [0, 0, 3e38, 640, 480], [3, 4, 1.25, 320, 240]]
    images = []
    for b, where in enumerate(("top", "bottom", "mixed", "top")):
        r = _rng(6000 + b)
        back = _rows(np.concatenate([r.uniform(150, 300, (nb, 2)), r.uniform(20, 80, (nb, 2))], 1), np.zeros(nb), r.integers(0, nc, nb), nc, r)
        sp = _rows(np.zeros((ns, 4)), np.zeros(ns), np.zeros(ns, np.int64), nc, r)
        sp[:, :4] = special[r.permutation(ns)] if b else special
        surv = np.concatenate([sp, back])
        ladder = _ladder(ns + nb, None, step=2.0 ** -10)          # descending
        if where == "top":
            surv[:, 4] = ladder
        elif where == "bottom":
            surv[:, 4] = np.concatenate([ladder[nb:], ladder[:nb]])
        else:
            surv[:, 4] = r.permutation(ladder)
        images.append(_embed(surv, 151, r))
    return _case(cid, images, {"special": ns, "background": nb}, nms_thr=nms_thr, adjust=adjust)


# ---- ties -----------------------------------------------------------------------------------------------------------------------------------
def ties():
    """[ties, ties_zero].  ties: 40 boxes of the chain geometry with ONE confidence, their positions along the row shuffled against their
    element order, so element order alone decides the picks.  ties_zero (prob_threshold 0): +0 and -0 confidences compare equal, yet the +0
    rows go first whatever the element order: rows 0..3 = (-0 at x 0), (+0 at x 3), (+0 at x 100), (-0 at x 103) pick rows 1 and 2."""
    nc = 2
    images = []
    for b in range(2):
        r = _rng(7000 + b)
        k = r.permutation(40)
        boxes = np.stack([3.0 * k, 0 * k, 10 + 0 * k, 10 + 0 * k], 1)
        label = np.zeros(40, np.int64) if b == 0 else (np.arange(40) % 7 == 0).astype(np.int64)
        images.append(_embed(_rows(boxes, np.full(40, 0.5), label, nc, r), 77, r, keep_order=True))
    out = [_case("ties", images, {"equal": 40}, distinct=False)]
    r = _rng(7100)
    surv = _rows([[0, 0, 10, 10], [3, 0, 10, 10], [100, 0, 10, 10], [103, 0, 10, 10]], [-0.0, 0.0, 0.0, -0.0], [0, 0, 0, 0], nc, r)
    img = _cold(11, nc, r, sign=-1.0)
    img[[1, 4, 6, 9]] = surv
    out.append(_case("ties_zero", [img], {"rows": [1, 4, 6, 9], "picked_rows": [4, 6]}, prob_thr=0.0, distinct=False))
    return out


# ---- the table ------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def cases():
    """id -> Case, built once per process"""
    out = [chain(130), chain(200), chain(130, True), chain(200, True)]
    out += [counts(c) for c in COUNTS] + [counts(257, nc=1)]
    out += [bins(nc) for nc in BINS_NC]
    out += [classes()] + equalities() + [geometry(), geometry(F(-0.5), "geometry_negthr")] + ties()
    for c in out:
        c.pred.setflags(write=False)
        c.adjust.setflags(write=False)
    ids = [c.id for c in out]
    assert len(set(ids)) == len(ids)
    return dict(zip(ids, out))


CASE_IDS = tuple(["chain_130", "chain_200", "chain2_130", "chain2_200"] + ["counts_%d" % c for c in COUNTS] + ["counts_257_nc1"]
                 + ["bins_%d" % nc for nc in BINS_NC]
                 + ["classes", "equalities_iou_eq", "equalities_iou_below", "equalities_conf_eq", "geometry", "geometry_negthr", "ties", "ties_zero"])


TIE_IDS = ("ties", "ties_zero")      # equal-comparing confidences: the reference's unstable quicksort has no single answer, the rule alone decides


@functools.lru_cache(maxsize=None)
def expected(cid, agnostic, adjusted):
    """the rule's answer for a case, computed once and shared (callers must not write to it): (list of dets per image, counts)"""
    c = cases()[cid]
    dets, cnt = postprocess(c.pred, c.prob_thr, c.nms_thr, bool(agnostic), c.adjust if adjusted else None)
    for d in dets:
        d.setflags(write=False)
    cnt.setflags(write=False)
    return dets, cnt
