"""The rule of include/si_obb.h in float64, plain numpy: ultralytics' nms_rotated with batch_probiou, stated exactly.

Candidates stand in the confidence order (descending confidence, ties by the earlier row).  A candidate is kept exactly when no EARLIER candidate
of the same label (any earlier one when agnostic) has !(probiou < nms_threshold): earlier candidates count even if they were dropped themselves
(the matrix form), a NaN drops the later box, the first candidate of a label always stays, different labels never interact (the exact statement
of what ultralytics' label * 7680 centre offset approximates).  The kernel makes the compare on the distance: iou >= thr <=> max(bd, eps) <=
-log(1 + eps - (1 - thr)^2); bd_compare() restates that form, pair_bd_f32() the kernel's fp32 operation order."""
import functools

import numpy as np

EPS = 1e-7
F = np.float32


def covariance(boxes):
    """boxes [k][5] = cx, cy, w, h, angle -> A, B, C of ultralytics' _get_covariance_matrix, in the dtype of `boxes`"""
    a, b = boxes[:, 2] ** 2 / 12, boxes[:, 3] ** 2 / 12
    cos, sin = np.cos(boxes[:, 4]), np.sin(boxes[:, 4])
    return a * cos ** 2 + b * sin ** 2, a * sin ** 2 + b * cos ** 2, (a - b) * cos * sin


def pair_bd(boxes):
    """bd[i][j] of box i (1) against box j (2) before the clamp, float64"""
    boxes = np.asarray(boxes, np.float64)
    with np.errstate(all="ignore"):
        A, B, C = covariance(boxes)
        x, y = boxes[:, 0], boxes[:, 1]
        sA, sB, sC = A[:, None] + A, B[:, None] + B, C[:, None] + C
        D = sA * sB - sC ** 2
        t1 = 0.25 * (sA * (y[:, None] - y) ** 2 + sB * (x[:, None] - x) ** 2) / (D + EPS)
        t2 = 0.5 * (sC * (x - x[:, None]) * (y[:, None] - y)) / (D + EPS)
        det = np.maximum(A * B - C ** 2, 0)
        det = np.where(np.isnan(A * B - C ** 2), np.nan, det)
        t3 = 0.5 * np.log(D / (4 * np.sqrt(det[:, None] * det) + EPS) + EPS)
        return t1 + t2 + t3


def iou_of_bd(bd):
    """float64; clamp(bd, eps, 100) hands a NaN on, as torch's does"""
    with np.errstate(all="ignore"):
        bd = np.asarray(bd, np.float64)
        c = np.where(np.isnan(bd), np.nan, np.clip(bd, EPS, 100.0))
        return 1 - np.sqrt(1 - np.exp(-c) + EPS)


def probiou(boxes):
    return iou_of_bd(pair_bd(boxes))


def bd_max(thr):
    return -np.log(1 + EPS - (1 - float(thr)) ** 2)


def bd_compare(bd, thr):
    """the compare the kernel makes: True where box 1 overlaps box 2"""
    with np.errstate(all="ignore"):
        return ~(np.where(bd < EPS, EPS, bd) > bd_max(thr))


def pair_bd_f32(boxes):
    """the kernel's arithmetic in numpy float32, operation by operation (include/si_obb.h); the transcendentals are numpy's"""
    b = np.asarray(boxes, F)
    e, q4, h2, h1, f4, f12 = F(EPS), F(0.25), F(0.5), F(1), F(4), F(12)
    with np.errstate(all="ignore"):
        va, vb = b[:, 2] * b[:, 2] / f12, b[:, 3] * b[:, 3] / f12
        c, s = np.cos(b[:, 4]), np.sin(b[:, 4])
        c2, s2 = c * c, s * s
        A, B, C = va * c2 + vb * s2, va * s2 + vb * c2, ((va - vb) * c) * s
        det = A * B - C * C
        det = np.where(det < 0, F(0), det)
        x, y = b[:, 0], b[:, 1]
        sA, sB, sC = A[:, None] + A, B[:, None] + B, C[:, None] + C
        D = sA * sB - sC * sC
        dx, dy = x[:, None] - x, y[:, None] - y
        r = h1 / (D + e)
        t12 = (q4 * (sA * (dy * dy) + sB * (dx * dx)) + h2 * ((sC * (x - x[:, None])) * dy)) * r
        q = D * (h1 / (f4 * np.sqrt(det[:, None] * det) + e)) + e
        out = t12 + h2 * np.log(q)
    assert out.dtype == F
    return out


def keep_mask(boxes, labels, thr, agnostic):
    """boxes in the confidence order -> the kept ones (bool [k])"""
    k = len(boxes)
    if k == 0:
        return np.zeros(0, bool)
    with np.errstate(all="ignore"):
        hit = ~(probiou(boxes) < thr)
    earlier = np.triu(np.ones((k, k), bool), 1)                      # [i][j]: i before j
    same = np.ones((k, k), bool) if agnostic else (np.asarray(labels)[:, None] == np.asarray(labels))
    return ~(hit & earlier & same).any(0)


# ---- the front end and the outputs -----------------------------------------------------------------------------------------------------------------
def candidates(pred, classes, extra, angle_off, prob_thr):
    """one image [rows][ne] (no box score) -> rows in the confidence order, their boxes [k][5] (fp32 bits), confidences, labels"""
    scores = pred[:, 4:4 + classes]
    label = scores.argmax(1)                                         # the first maximum
    conf = scores[np.arange(len(pred)), label]
    rows = np.nonzero(conf >= F(prob_thr))[0]
    rows = rows[np.argsort(-conf[rows].astype(np.float64), kind="stable")]
    boxes = np.concatenate([pred[rows, :4], pred[rows, 4 + classes + angle_off][:, None]], 1)
    return rows, boxes, conf[rows], label[rows]


def postprocess(pred, classes, extra, angle_off, prob_thr, nms_thr, agnostic, max_det=None, adjust=None):
    """pred [n][rows][ne] fp32 -> per image (obbs [k][7] fp32, src_rows, extras), and the uncapped counts"""
    outs, counts = [], []
    for b, p in enumerate(np.asarray(pred, F)):
        rows, boxes, conf, label = candidates(p, classes, extra, angle_off, prob_thr)
        keep = keep_mask(boxes, label, nms_thr, agnostic)
        counts.append(int(keep.sum()))
        rows, boxes, conf, label = (v[keep][:max_det] for v in (rows, boxes, conf, label))
        box = boxes.copy()
        if adjust is not None:
            pad_l, pad_t, scale = (F(v) for v in np.asarray(adjust, F).reshape(-1, 5)[b, :3])
            with np.errstate(all="ignore"):
                box[:, 0], box[:, 1] = (box[:, 0] - pad_l) / scale, (box[:, 1] - pad_t) / scale
                box[:, 2], box[:, 3] = box[:, 2] / scale, box[:, 3] / scale
        obbs = np.concatenate([box, conf[:, None], label[:, None].astype(F)], 1).astype(F).reshape(-1, 7)
        outs.append((obbs, rows.astype(np.int32), p[rows, 4 + classes:]))
    return outs, np.asarray(counts, np.int32)


# ---- the seeded box maker ------------------------------------------------------------------------------------------------------------------------
def make_boxes(seed, k):
    """k oriented boxes, half of them jittered copies of the others, at a density that does not depend on k"""
    r = np.random.Generator(np.random.Philox(seed))
    side = 60.0 * np.sqrt(max(k, 1))
    base = np.stack([r.uniform(0, side, k), r.uniform(0, side, k), r.uniform(30, 90, k), r.uniform(10, 40, k), r.uniform(-1.6, 1.6, k)], 1)
    twin = r.integers(0, max(k // 2, 1), k)
    copy = np.arange(k) >= (k + 1) // 2
    base[copy] = base[twin[copy]] + r.normal(0, 1, (int(copy.sum()), 5)) * np.asarray([6, 6, 5, 3, 0.15])
    return base.astype(F)


def make_pred(seed, k, classes, extra, angle_off, below=37):
    """one image: k rows above the threshold 0.25 with distinct confidences (2^-13 apart) and `below` rows under it, shuffled; the payload
    beside the angle holds arbitrary bits (NaNs among them)"""
    r = np.random.Generator(np.random.Philox(seed + 1000003))
    rows = k + below
    boxes = np.concatenate([make_boxes(seed, k), make_boxes(seed + 7, below)])
    conf = np.concatenate([F(0.3) + F(2.0 ** -13) * r.permutation(k).astype(F), r.uniform(0.01, 0.2, below).astype(F)])
    label = r.integers(0, classes, rows)
    pred = np.zeros((rows, 4 + classes + extra), F)
    pred[:, :4] = boxes[:, :4]
    pred[:, 4:4 + classes] = conf[:, None] * r.uniform(0.1, 0.9, (rows, classes)).astype(F)
    pred[np.arange(rows), 4 + label] = conf
    payload = r.integers(0, 2 ** 32, (rows, extra), dtype=np.uint64).astype(np.uint32).view(F)
    pred[:, 4 + classes:] = payload
    pred[:, 4 + classes + angle_off] = boxes[:, 4]
    return pred[r.permutation(rows)]


@functools.lru_cache(maxsize=None)
def case(seed, counts, classes, extra=1, angle_off=0):
    """pred [n][rows][ne] with counts[b] candidates in image b (rows = max(counts) + 37 everywhere); treat as read-only"""
    rows = max(counts) + 37
    pred = np.stack([make_pred(seed + 101 * b, c, classes, extra, angle_off, rows - c) for b, c in enumerate(counts)])
    pred.setflags(write=False)
    return pred


def deviation_and_gap(pred, classes, extra, angle_off, prob_thr, nms_thr):
    """over every candidate pair of every image: the largest |iou(fp32 bd) - iou(float64 bd)|, and the smallest |float64 iou - nms_thr| (NaN
    pairs, which both decide alike, left out)"""
    dev, gap = 0.0, np.inf
    for p in np.asarray(pred, F):
        _, boxes, _, _ = candidates(p, classes, extra, angle_off, prob_thr)
        if len(boxes) < 2:
            continue
        i64 = probiou(boxes)
        i32 = iou_of_bd(pair_bd_f32(boxes))
        ok = np.triu(np.ones(i64.shape, bool), 1) & ~np.isnan(i64)
        assert not np.isnan(i32[ok]).any()
        if ok.any():
            dev, gap = max(dev, float(np.abs(i32 - i64)[ok].max())), min(gap, float(np.abs(i64 - nms_thr)[ok].min()))
    return dev, gap
