"""The general detection post-processing rule (include/si_detect.h) and its cases, in numpy fp32, no GPU.

THE RULE is the one of tests/post_reference.py -- its sort_order, nms, finish and clip are imported, not restated -- behind a general front
end: `filter_rows(pred, desc)` reads a head without a box score (confidence = the first-maximum class score, strict '>' from -FLT_MAX, so a
row with no maximum has label -1 and confidence -FLT_MAX), corner boxes ({x0, y0, x1 - x0, y1 - y0}) and a payload of `extra` elements behind
the class scores, which is never interpreted: `postprocess` returns it, the prediction row and the network box of every pick beside the
rows post_reference.postprocess returns.  `masks_ref` is ultralytics' process_mask without the upsample: crop && dot > 0, the dot in index
order with every product and sum rounded to fp32 on its own.

A pred here is always the LOGICAL rows form [n][rows][ne]; the channel-major layout is a transposition of the storage and has no rule of its
own (to_channels).

THE CASES.  cases() converts post_reference.cases() where the conversion keeps the case's structure and adds generators where it cannot:
  v5/<id>     the case as it is (box score, cx cy w h)
  v5xy/<id>   corner boxes: the columns hold fp32 x0, y0, x1, y1 as the rule forms them, so the boxes keep their BITS (every id)
  v8/<id>     no box score: class score k becomes fl(box score * class score k), and a row that had no class maximum keeps none.  The
              survivors are then the original's with label >= 0, bit for bit (test_detect_post_cpu.py asserts it) -- for every id but
              `classes`, whose +inf / NaN box scores have no counterpart
  v8xy/<id>   both
  v8_classes  what the class scan does at its edges without a box score: tied maxima, NaN among the scores, a +inf score, rows with no
              maximum (dropped at a finite threshold)
  v8_minus_one  prob_threshold = -inf: rows with no maximum survive with confidence -FLT_MAX and label -1 and compete with one another
  sized_*     rows in {1, 127, 128, 129, 257}, zero survivors, one lane-walk of 1300 elements: the sizes of the filter kernels"""
import functools
from typing import NamedTuple, Optional

import numpy as np

import post_reference as pr
from post_reference import F, FLT_MAX, assert_same, assert_same_result, clip, finish, nms, sort_order  # noqa: F401  (the rule's other half)


class Desc(NamedTuple):
    classes: int
    objectness: int = 0
    extra: int = 0
    box_format: str = "cxcywh"
    prob_thr: np.float32 = pr.PROB_THR
    nms_thr: np.float32 = pr.NMS_THR
    agnostic: bool = False

    @property
    def ne(self):
        return 4 + self.objectness + self.classes + self.extra


# ---- the rule -----------------------------------------------------------------------------------------------------------------------------
def filter_rows(pred, desc):
    """pred [rows][ne] -> (element index, box [k][4] = x, y, w, h, label, confidence) of the survivors, element order"""
    p = np.ascontiguousarray(pred, F)
    rows, ne = p.shape
    assert ne == desc.ne, (ne, desc)
    first = 4 + desc.objectness
    score = np.full(rows, -FLT_MAX, F)
    label = np.full(rows, -1, np.int32)
    for k in range(desc.classes):
        s = p[:, first + k]
        up = s > score
        label[up] = k
        score[up] = s[up]
    conf = p[:, 4] * score if desc.objectness else score
    keep = np.nonzero(conf >= F(desc.prob_thr))[0]
    a, b, c, d = (p[keep, i] for i in range(4))
    if desc.box_format == "cxcywh":
        x0, y0 = a - c * F(0.5), b - d * F(0.5)
        x1, y1 = a + c * F(0.5), b + d * F(0.5)
    else:
        assert desc.box_format == "xyxy"
        x0, y0, x1, y1 = a, b, c, d
    return keep, np.stack([x0, y0, x1 - x0, y1 - y0], 1).astype(F), label[keep], conf[keep]


class Picks(NamedTuple):
    dets: np.ndarray        # [k][6], what post_reference.finish returns
    src_rows: np.ndarray    # [k] int32
    net_boxes: np.ndarray   # [k][4]
    extras: np.ndarray      # [k][extra], the payload's bits


def postprocess_image(pred, desc, adjust=None):
    with np.errstate(all="ignore"):
        elem, box, label, conf = filter_rows(pred, desc)
        o = sort_order(elem, conf)
        elem, box, label, conf = elem[o], box[o], label[o], conf[o]
        p = nms(box, label, desc.nms_thr, desc.agnostic)
        rows = elem[p].astype(np.int32)
        payload = np.ascontiguousarray(np.ascontiguousarray(pred, F)[rows, desc.ne - desc.extra:])
        return Picks(finish(box[p], label[p], conf[p], adjust), rows, np.ascontiguousarray(box[p]), payload)


def postprocess(pred, desc, adjust=None):
    """pred [n][rows][ne] -> (list of Picks per image, counts int32 [n]); no cap: max_det only cuts these lists"""
    outs = [postprocess_image(pred[b], desc, None if adjust is None else adjust[b]) for b in range(len(pred))]
    return outs, np.asarray([len(o.dets) for o in outs], np.int32)


def to_channels(pred):
    """the logical rows form [n][rows][ne] as a channel-major export stores it: [n][ne][rows]"""
    return np.ascontiguousarray(np.transpose(np.asarray(pred, F), (0, 2, 1)))


def assert_same_bits(got, ref, what=""):
    """equality of the 32-bit words, NaN payloads included (the payload is carried, never computed)"""
    got, ref = np.ascontiguousarray(got), np.ascontiguousarray(ref)
    assert got.shape == ref.shape and got.dtype.itemsize == ref.dtype.itemsize == 4, (what, got.shape, ref.shape, got.dtype, ref.dtype)
    g, r = got.view(np.uint32), ref.view(np.uint32)
    bad = g != r
    assert not bad.any(), "%s: %d of %d words differ, first at %s: %08x, expected %08x" % (
        what, int(bad.sum()), r.size, tuple(np.argwhere(bad)[0]), g[bad][0], r[bad][0])


def assert_same_picks(got, ref, max_det=None, what=""):
    """got: a hipops.DetectResult (or anything with its fields); ref: postprocess's return.  Every output the result holds is compared."""
    outs, cnt = ref
    assert list(got.counts) == list(cnt), "%s: counts %s, expected %s" % (what, list(got.counts), list(cnt))
    for b, o in enumerate(outs):
        k = len(o.dets) if max_det is None else min(len(o.dets), max_det)
        assert_same(got.dets[b], o.dets[:k], "%s image %d dets" % (what, b))
        if got.src_rows is not None:
            assert list(got.src_rows[b]) == list(o.src_rows[:k]), "%s image %d src_rows" % (what, b)
        if got.net_boxes is not None:
            assert_same(got.net_boxes[b], o.net_boxes[:k], "%s image %d net_boxes" % (what, b))
        if got.extras is not None:
            assert_same_bits(got.extras[b], o.extras[:k], "%s image %d extras" % (what, b))


# ---- masks --------------------------------------------------------------------------------------------------------------------------------
def mask_dots(protos, coef):
    """protos [mh][mw][nm], coef [nm] -> (((0 + c0 p0) + c1 p1) + ...) per pixel, every product and every sum an fp32 operation"""
    acc = np.zeros(protos.shape[:2], F)
    with np.errstate(all="ignore"):
        for k in range(len(coef)):
            acc = acc + F(coef[k]) * protos[:, :, k]
    assert acc.dtype == F
    return acc


def mask_crop(box, mh, mw, ratio_w, ratio_h):
    with np.errstate(all="ignore"):
        bx, by, bw, bh = (F(v) for v in box)
        x1, x2 = bx * F(ratio_w), (bx + bw) * F(ratio_w)
        y1, y2 = by * F(ratio_h), (by + bh) * F(ratio_h)
        c = np.arange(mw, dtype=F)[None, :]
        r = np.arange(mh, dtype=F)[:, None]
        return (c >= x1) & (c < x2) & (r >= y1) & (r < y2)


def masks_ref(protos, extras, net_boxes, counts, ratio_w, ratio_h, coef_off=0, nm=None):
    """protos [n][mh][mw][nm'], extras [n][max_det][extra], net_boxes [n][max_det][4], counts [n] -> per image [min(count, max_det)][mh][mw]
    uint8"""
    protos = np.ascontiguousarray(protos, F)
    n, mh, mw, pnm = protos.shape
    nm = pnm if nm is None else nm
    max_det = extras.shape[1]
    out = []
    for b in range(n):
        k = min(int(counts[b]), max_det)
        planes = np.zeros((k, mh, mw), np.uint8)
        for d in range(k):
            dot = mask_dots(protos[b][:, :, :nm], np.asarray(extras[b, d, coef_off:coef_off + nm], F))
            planes[d] = mask_crop(net_boxes[b, d], mh, mw, ratio_w, ratio_h) & (dot > 0)
        out.append(planes)
    return out


# ---- conversions ----------------------------------------------------------------------------------------------------------------------------
class DCase(NamedTuple):
    id: str
    pred: np.ndarray        # [n][rows][ne], logical rows form, no payload
    desc: Desc              # extra = 0, agnostic left to the test
    adjust: np.ndarray      # [n][5]
    origin: Optional[str]   # the post_reference case this one converts
    facts: dict


def with_payload(pred, extra, seed=0, nan=False):
    """pred with `extra` random payload elements behind every row; nan: quiet and signalling NaNs with a different payload in every element"""
    n, rows, ne = pred.shape
    r = np.random.Generator(np.random.Philox(9000 + seed))
    if nan:
        bits = (np.arange(n * rows * extra, dtype=np.uint32) * np.uint32(2654435761) & np.uint32(0x007fffff)) | np.uint32(1)
        bits |= np.where(np.arange(bits.size) % 2 == 0, np.uint32(0x7f800000), np.uint32(0xff800000))
        pay = bits.view(F).reshape(n, rows, extra)
    else:
        pay = r.uniform(-4, 4, (n, rows, extra)).astype(F)
    return np.ascontiguousarray(np.concatenate([np.asarray(pred, F), pay], 2))


def to_xyxy(pred):
    """the box columns as fp32 corners, formed as the rule forms them: the resulting boxes have the original's bits"""
    p = np.array(pred, F)
    with np.errstate(all="ignore"):
        cx, cy, w, h = (p[..., i].copy() for i in range(4))
        p[..., 0], p[..., 1] = cx - w * F(0.5), cy - h * F(0.5)
        p[..., 2], p[..., 3] = cx + w * F(0.5), cy + h * F(0.5)
    return p


def to_noobj(pred):
    """[.., 5 + nc] -> [.., 4 + nc]: class score k = fl(box score * class score k); a row without a class maximum keeps none (-inf)"""
    p = np.asarray(pred, F)
    with np.errstate(all="ignore"):
        cls = (p[..., 4:5] * p[..., 5:]).astype(F)
    none = ~(p[..., 5:] > -FLT_MAX).any(-1)
    cls[none] = -np.inf
    return np.ascontiguousarray(np.concatenate([p[..., :4], cls], -1))


NO_V8 = ("classes",)        # its +inf / NaN / zero box scores have no counterpart without a box score


def _sized(cid, rows, survivors, classes, objectness, seed, n=2):
    """`survivors` random dense boxes with distinct confidences among rows - survivors dropped rows"""
    assert survivors <= rows
    r = np.random.Generator(np.random.Philox(8000 + seed))
    images = []
    for b in range(n):
        k = survivors
        boxes = np.concatenate([r.uniform(0, 100, (k, 2)), r.uniform(20, 80, (k, 2))], 1)
        label = r.integers(0, 6, k) * max(1, (classes - 1) // 5)     # at most six labels, spread up to the last class: real per-class suppression
        surv = pr._rows(boxes, pr._ladder(k, r) if k else np.zeros(0), np.minimum(label, classes - 1), classes, r)
        images.append(pr._embed(surv, rows, r) if k else pr._cold(rows, classes, r))
    pred = np.ascontiguousarray(np.stack(images), F)
    if not objectness:
        pred = to_noobj(pred)
    return DCase(cid, pred, Desc(classes, objectness), pr._adjust(n), None, {"rows": rows, "survivors": survivors})


def _v8_classes():
    nc = 4
    inf, nan = np.inf, np.nan
    # (class scores, box, expected label or None when the row is dropped at 0.25)
    table = [
        ([0.5, 0.9, 0.9, 0.3], (50, 50, 20, 20), 1),                    # tied maxima: the first wins
        ([0.8, 0.8, 0.8, 0.8], (90, 50, 20, 20), 0),
        ([0.1, 0.2, 0.3, inf], (130, 50, 20, 20), 3),                   # +inf: first
        ([nan, 0.7, nan, 0.2], (250, 50, 20, 20), 1),                   # NaN never wins a compare
        ([nan] * 4, (300, 300, 20, 20), None),                          # no maximum: label -1, confidence -FLT_MAX, dropped
        ([-inf] * 4, (300, 300, 20, 20), None),
        ([-FLT_MAX] * 4, (290, 50, 20, 20), None),                      # not > -FLT_MAX
        ([0.2, 0.6, -inf, 0.6], (370, 50, 20, 20), 1),
        ([0.25, 0.1, 0.1, 0.1], (410, 50, 20, 20), 0),                  # equal to the threshold: kept
        ([np.nextafter(F(0.25), F(0)), 0.1, 0.1, 0.1], (450, 50, 20, 20), None),
    ]
    images = []
    for b in range(2):
        r = np.random.Generator(np.random.Philox(8100 + b))
        special = np.asarray([[x + w * 0.5, y + h * 0.5, w, h] + cs for cs, (x, y, w, h), _ in table], F)
        m = 40
        back = to_noobj(pr._rows(np.concatenate([r.uniform(0, 200, (m, 2)) + 100, r.uniform(20, 80, (m, 2))], 1), pr._ladder(m, r),
                                 r.integers(0, nc, m), nc, r)[None])[0]
        surv = np.concatenate([special, back] if b == 0 else [back, special[::-1]])
        cold = to_noobj(pr._cold(101, nc, r)[None])[0]
        pos = r.permutation(np.sort(r.choice(101, len(surv), replace=False)))
        cold[pos] = surv
        images.append(cold)
    want = sorted(t[2] for t in table if t[2] is not None)
    return DCase("v8_classes", np.ascontiguousarray(np.stack(images), F), Desc(nc, 0), pr._adjust(2), None,
                 {"special_labels": want, "dropped": sum(t[2] is None for t in table), "background": 40})


def _v8_minus_one():
    """prob_threshold -inf: every row survives, also those with no maximum (six of them, two pairs sharing a box)"""
    base = _v8_classes()
    d = base.desc._replace(prob_thr=F(-np.inf))
    return DCase("v8_minus_one", base.pred, d, base.adjust, None, {"minus_one": 3, "rows": 101})


@functools.lru_cache(maxsize=None)
def cases():
    out = []
    for cid, c in pr.cases().items():
        nc = c.pred.shape[2] - 5
        d5 = Desc(nc, 1, 0, "cxcywh", c.prob_thr, c.nms_thr)
        out.append(DCase("v5/" + cid, c.pred, d5, c.adjust, cid, c.facts))
        out.append(DCase("v5xy/" + cid, to_xyxy(c.pred), d5._replace(box_format="xyxy"), c.adjust, cid, c.facts))
        if cid not in NO_V8:
            d8 = d5._replace(objectness=0)
            out.append(DCase("v8/" + cid, to_noobj(c.pred), d8, c.adjust, cid, c.facts))
            out.append(DCase("v8xy/" + cid, to_noobj(to_xyxy(c.pred)), d8._replace(box_format="xyxy"), c.adjust, cid, c.facts))
    out += [_v8_classes(), _v8_minus_one()]
    for rows in (1, 127, 128, 129, 257):
        out.append(_sized("sized_rows%d" % rows, rows, min(rows, 33), 3, rows % 2, rows))
    out.append(_sized("sized_none", 129, 0, 5, 0, 1))
    out.append(_sized("sized_none_v5", 257, 0, 2, 1, 2))
    out.append(_sized("sized_lvis", 300, 70, 1264, 0, 3))          # ne = 1300 with a payload of 32
    out.append(_sized("sized_ne128", 200, 70, 92, 0, 4))           # ne = 128 with a payload of 32
    for c in out:
        c.pred.setflags(write=False)
    ids = [c.id for c in out]
    assert len(set(ids)) == len(ids)
    return dict(zip(ids, out))


@functools.lru_cache(maxsize=None)
def expected(cid, agnostic=False, adjusted=False, extra=0, nan_payload=False):
    """the rule's answer for a case with a payload of `extra` elements, computed once and shared: (pred with payload, list of Picks, counts)"""
    c = cases()[cid]
    pred = with_payload(c.pred, extra, seed=len(cid), nan=nan_payload) if extra else c.pred
    outs, cnt = postprocess(pred, c.desc._replace(extra=extra, agnostic=bool(agnostic)), c.adjust if adjusted else None)
    pred.setflags(write=False)
    cnt.setflags(write=False)
    return pred, outs, cnt


# ---- mask cases -----------------------------------------------------------------------------------------------------------------------------
class MCase(NamedTuple):
    id: str
    protos: np.ndarray      # [n][mh][mw][nm]
    extras: np.ndarray      # [n][max_det][extra]
    net_boxes: np.ndarray   # [n][max_det][4]
    counts: np.ndarray      # [n]
    ratio_w: np.float32
    ratio_h: np.float32
    coef_off: int


SUB = np.float32(1.401298464324817e-45)      # the smallest subnormal

MASK_SIZES = ((1, 1), (5, 7), (16, 16), (20, 24))
MASK_NM = (1, 3, 32, 33, 64)


def mask_boxes(mh, mw, ratio_w, ratio_h, r, k):
    """k boxes in network coordinates around a mh x mw mask: inside, across each border, outside, empty, inverted, NaN, edges on integers, then
    random ones"""
    W, H = mw / float(ratio_w), mh / float(ratio_h)
    fixed = [
        (0.25 * W, 0.25 * H, 0.5 * W, 0.5 * H),               # inside
        (-0.3 * W, 0.2 * H, 0.6 * W, 0.5 * H),                # across the left border
        (0.7 * W, 0.2 * H, 0.6 * W, 0.5 * H),                 # right
        (0.2 * W, -0.3 * H, 0.5 * W, 0.6 * H),                # top
        (0.2 * W, 0.7 * H, 0.5 * W, 0.6 * H),                 # bottom
        (-0.1 * W, -0.1 * H, 1.2 * W, 1.2 * H),               # around everything
        (2 * W, 2 * H, 0.5 * W, 0.5 * H),                     # outside
        (0.5 * W, 0.5 * H, 0.0, 0.0),                         # empty
        (0.75 * W, 0.75 * H, -0.5 * W, -0.5 * H),             # inverted
        (np.nan, 0.2 * H, 0.5 * W, 0.5 * H), (0.2 * W, 0.2 * H, np.nan, 0.5 * H), (0.2 * W, np.inf, 0.5 * W, 0.5 * H),
        (1.0 / float(ratio_w), 1.0 / float(ratio_h), 2.0 / float(ratio_w), 2.0 / float(ratio_h)),     # edges exactly on pixels 1 and 3
        (0.0, 0.0, W, H),
    ]
    rnd = [(r.uniform(-0.2, 0.9) * W, r.uniform(-0.2, 0.9) * H, r.uniform(0.05, 0.6) * W, r.uniform(0.05, 0.6) * H) for _ in range(max(0, k - len(fixed)))]
    return np.asarray((fixed + rnd)[:k], F)


def mask_case(cid, n, mh, mw, nm, counts, max_det, seed, extra=None, coef_off=0, ratio=(0.25, 0.25), zeros=False):
    """prototypes and coefficients in [-1, 1]; zeros: pixels whose dot is exactly 0 and the smallest subnormal either side (detections 0..2 of
    every image: coefficients (1, 0, ..), prototype 0 of the first pixels = 0, +SUB, -SUB, -0)"""
    r = np.random.Generator(np.random.Philox(8500 + seed))
    extra = nm + coef_off if extra is None else extra
    protos = r.uniform(-1, 1, (n, mh, mw, nm)).astype(F)
    extras = r.uniform(-1, 1, (n, max_det, extra)).astype(F)
    boxes = np.stack([mask_boxes(mh, mw, ratio[0], ratio[1], r, max_det) for _ in range(n)])
    if zeros:
        flat = protos.reshape(n, mh * mw, nm)
        vals = [F(0), SUB, -SUB, F(-0.0)]
        for i, v in enumerate(vals[:mh * mw]):
            flat[:, i, 0] = v
        protos = flat.reshape(n, mh, mw, nm)
        for d in range(min(3, max_det)):
            extras[:, d, coef_off:coef_off + nm] = 0
            extras[:, d, coef_off] = (1.0, -1.0, 0.5)[d]
            boxes[:, d] = (0.0, 0.0, mw / ratio[0], mh / ratio[1])
    return MCase(cid, protos, extras, boxes, np.asarray(counts, np.int32), F(ratio[0]), F(ratio[1]), coef_off)


@functools.lru_cache(maxsize=None)
def mask_cases():
    out = []
    seed = 0
    for (mh, mw) in MASK_SIZES:
        for nm in MASK_NM:
            seed += 1
            max_det = 16
            counts = (0, 1, max_det, max_det + 5)
            out.append(mask_case("m%dx%d_nm%d" % (mh, mw, nm), 4, mh, mw, nm, counts, max_det, seed, coef_off=seed % 3, zeros=(nm in (1, 32))))
    out.append(mask_case("m160x160_nm32", 2, 160, 160, 32, (3, 20), 16, 99, extra=37, coef_off=5))
    out.append(mask_case("m20x24_nm32_ratio", 2, 20, 24, 32, (16, 7), 16, 98, ratio=(24 / 96.0, 20 / 64.0)))
    out.append(mask_case("m5x7_nm3_maxdet1", 2, 5, 7, 3, (1, 0), 1, 97))
    return {c.id: c for c in out}


@functools.lru_cache(maxsize=None)
def mask_expected(cid):
    c = mask_cases()[cid]
    return masks_ref(c.protos, c.extras, c.net_boxes, c.counts, c.ratio_w, c.ratio_h, c.coef_off, c.protos.shape[3])
