"""CPU pin of tests/post_reference.py (no GPU): the numpy rule against the C oracle (orc.yolo_postprocess, the restatement of
test_yolo.cpp:337-428) bit for bit on every generated case whose confidences are distinct -- the oracle's quicksort is unstable, so the tie
cases have no answer there -- and each generator's structural promise asserted from the rule alone, so that a generator which no longer reaches
the boundary it was written for fails here.  Also here: the two wrong rules the cases exist to catch (suppression by any earlier candidate;
the intersection with fmaxf / fminf semantics, which is what the kernel computed before this matrix) DO differ on them; both live in this
file, the rule has one form."""
import numpy as np
import pytest

import post_reference as pr

F = np.float32


def _nms_with(big, small, any_earlier=False):
    """a greedy NMS that is NOT the rule: the intersection's max / min are `big` / `small` (np.fmax / np.fmin: fmaxf / fminf, the non-NaN
    operand wins -- what the kernel computed before this matrix); any_earlier: suppress by ANY earlier candidate instead of any earlier
    PICKED one.  The rule itself (post_reference.nms) has one form; these exist to show that the cases see the difference."""
    def nms(box, label, nms_threshold, agnostic):
        x, y, x2, y2 = box[:, 0], box[:, 1], box[:, 0] + box[:, 2], box[:, 1] + box[:, 3]
        area = box[:, 2] * box[:, 3]
        seen, picks = [], []
        for i in range(len(box)):
            keep = True
            if seen:
                j = np.asarray(seen)
                w = small(x2[i], x2[j]) - big(x[i], x[j])
                h = small(y2[i], y2[j]) - big(y[i], y[j])
                ia = np.where((w <= 0) | (h <= 0), F(0), w * h)
                s = ia / (area[i] + area[j] - ia) > F(nms_threshold)
                if not agnostic:
                    s &= label[j] == label[i]
                keep = not s.any()
            if keep:
                picks.append(i)
            if keep or any_earlier:
                seen.append(i)
        return np.asarray(picks, np.int64)
    return nms


ANY_EARLIER = _nms_with(pr.sel_gt, pr.sel_lt, any_earlier=True)
FMAX_FMIN = _nms_with(np.fmax, np.fmin)


def _picked_rows(case, b, agnostic, nms=pr.nms):
    """element indices (rows of the prediction) of image b's picks, in picked order"""
    with np.errstate(all="ignore"):
        elem, box, label, conf = pr.filter_rows(case.pred[b], case.prob_thr)
        o = pr.sort_order(elem, conf)
        p = nms(box[o], label[o], case.nms_thr, agnostic)
    return elem[o][p], box[o][p], label[o][p]


def test_the_table_is_complete():
    assert tuple(pr.cases()) == pr.CASE_IDS
    for c in pr.cases().values():
        n, rows, ne = c.pred.shape
        assert c.adjust.shape == (n, 5) and rows % 128 != 0 and ne >= 6, c.id
        assert rows <= 2400, "the largest input is 2049 candidates in about 2300 rows"


@pytest.mark.parametrize("adjusted", [False, True], ids=["raw", "adjust"])
@pytest.mark.parametrize("agnostic", [False, True], ids=["perclass", "agnostic"])
@pytest.mark.parametrize("cid", [c for c in pr.CASE_IDS if c not in pr.TIE_IDS])
def test_rule_equals_the_c_oracle(orc, cid, agnostic, adjusted):
    c = pr.cases()[cid]
    assert c.distinct and all(len(np.unique(cf)) == len(cf) for _, cf in pr.survivors(c.pred, c.prob_thr)), "confidences must be distinct here"
    ref = orc.yolo_postprocess(c.pred, float(c.prob_thr), float(c.nms_thr), agnostic, c.adjust if adjusted else None)
    pr.assert_same_result(pr.expected(cid, agnostic, adjusted), ref, cid)


# ---- structural promises --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("length", [130, 200])
def test_chain_picks_every_second_box_and_straddles_the_chunk(length):
    c = pr.cases()["chain_%d" % length]
    lane63 = []
    for phase in range(4):
        for agnostic in (False, True):
            _, box, _ = _picked_rows(c, phase, agnostic)
            iso, ch = box[box[:, 1] == 1000], box[box[:, 1] == 0]
            assert len(iso) == phase
            assert list(ch[:, 0]) == [3.0 * k for k in range(0, length, 2)], "every second box of the chain"
            # the wrong rule keeps the head of the chain and every box that clears ALL earlier ones: a different answer
            _, wrong, _ = _picked_rows(c, phase, agnostic, nms=ANY_EARLIER)
            assert len(wrong) < len(box)
        labels, conf = pr.survivors(c.pred[phase:phase + 1], c.prob_thr)[0]
        assert len(conf) == phase + length > 128 and (np.diff(conf) < 0).all()
        lane63.append((63 - phase) % 2 == 0)          # sorted position 63 is chain box 63 - phase: alive when that is even
    assert lane63 == [False, True, False, True], "candidate 63 alive in one variant and dead in another"
    # neighbour and next-but-one IoU, in fp32, either side of the threshold
    assert F(70) / F(130) > c.nms_thr > F(40) / F(160)


@pytest.mark.parametrize("length", [130, 200])
def test_interleaved_chains_interact_only_when_agnostic(length):
    c = pr.cases()["chain2_%d" % length]
    for phase in range(4):
        _, box, label = _picked_rows(c, phase, False)
        for lab in (0, 1):
            ch = box[(label == lab) & (box[:, 1] == 0)]
            assert list(ch[:, 0]) == [3.0 * k + lab for k in range(0, length, 2)], "per class each chain is on its own"
        _, abox, alabel = _picked_rows(c, phase, True)
        assert len(abox) < len(box) and set(alabel[abox[:, 1] == 0]) == {0, 1}, "agnostic: they suppress one another"


@pytest.mark.parametrize("count", pr.COUNTS)
def test_counts_are_the_listed_ones_and_the_picked_lists_cross_64_and_256(count):
    c = pr.cases()["counts_%d" % count]
    for b, (label, conf) in enumerate(pr.survivors(c.pred, c.prob_thr)):
        assert len(conf) == count and len(np.unique(conf)) == count, pr.LAYOUTS[b]
    for agnostic in (False, True):
        dets, cnt = pr.expected(c.id, agnostic, False)
        assert cnt[0] == count and cnt[1] == 1 and 1 <= cnt[2] <= count
        if count >= 65:
            assert 1 < cnt[2] < count, "random dense: real suppression"
    far_labels = pr.expected(c.id, False, False)[0][0][:, 5]
    per_label = np.bincount(far_labels.astype(np.int64), minlength=3)
    if count >= 257:
        assert per_label.max() > 64, "a per-class picked list longer than one chunk"
    if count >= 1023:
        assert per_label.min() > 256, "every per-class picked list longer than 256"


def test_counts_cover_both_sides_of_every_structural_size():
    for edge in (64, 128, 256, 1024):
        assert {edge - 1, edge, edge + 1} <= set(pr.COUNTS)
    assert 2049 in pr.COUNTS and 1 in pr.COUNTS
    c = pr.cases()["counts_257_nc1"]
    assert c.pred.shape[2] == 6


@pytest.mark.parametrize("nc", pr.BINS_NC)
def test_bins_reach_their_boundaries(nc):
    c = pr.cases()["bins_%d" % nc]
    assert c.pred.shape[2] == nc + 5
    dets, cnt = pr.expected(c.id, False, False)
    for b, (label, conf) in enumerate(pr.survivors(c.pred, c.prob_thr)):
        heavy = c.facts["heavy"][b]
        cand = np.bincount(label + 1, minlength=nc + 1)
        assert cand[heavy + 1] == 82 > 64 and cand[nc] > 0, "a segment longer than a chunk; the last bin is never empty"
        if nc > 2:
            assert (cand[1:] == 0).any(), "some labels are empty"
        assert cand[0] == b, "image 1 holds one label -1 row"
        picks = np.bincount(dets[b][:, 5].astype(np.int64) + 1, minlength=nc + 1)
        assert picks[heavy + 1] > 64, "more than 64 picks under one label"
    assert {63, 64, 65} <= set(pr.BINS_NC), "64, 65 and 66 bins: the lane-strided prefix"
    assert max(pr.BINS_NC) + 5 == 128, "ne = 128 is the filter's LDS limit"


def test_classes_label_minus_one_nan_and_inf():
    c = pr.cases()["classes"]
    for b, (label, conf) in enumerate(pr.survivors(c.pred, c.prob_thr)):
        assert len(conf) == len(c.facts["special_labels"]) + c.facts["background"], "NaN confidences and negative ones are dropped"
        assert np.isposinf(conf[0]) and np.isfinite(conf[1:]).all() and label[0] == 3, "+inf first"
        assert (label == -1).sum() == 4
        assert not np.isnan(conf).any()
    for agnostic in (False, True):
        dets, cnt = pr.expected(c.id, agnostic, False)
        for d in dets:
            minus = d[d[:, 5] == -1]
            assert len(minus) == 3, "two label -1 rows share a box: the second goes"
            assert minus[0, 4] == pr.FLT_MAX
            assert np.isposinf(d[0, 4])
    # tied maxima: the first one wins
    with np.errstate(all="ignore"):
        _, _, label, _ = pr.filter_rows(np.asarray([[0, 0, 1, 1, 1.0, 0.5, 0.9, 0.9, 0.3], [0, 0, 1, 1, 1.0, 0.9, 0.9, 0.9, 0.9]], F), 0.25)
    assert list(label) == [1, 0]


def test_equalities_flip_with_one_ulp():
    cs = pr.cases()
    eq, below, conf = cs["equalities_iou_eq"], cs["equalities_iou_below"], cs["equalities_conf_eq"]
    assert eq.nms_thr == F(8) / F(24) and below.nms_thr == np.nextafter(eq.nms_thr, F(0)) and np.array_equal(eq.pred, below.pred)
    for agnostic in (False, True):
        d_eq, d_below = pr.expected(eq.id, agnostic, False)[0][0], pr.expected(below.id, agnostic, False)[0][0]
        assert len(d_eq) == 2 and len(d_below) == 1
        assert [tuple(r) for r in d_eq[:, :4]] == [(0, 0, 4, 4), (2, 0, 4, 4)]
        d = pr.expected(conf.id, agnostic, False)[0][0]
        assert len(d) == 2 and d[:, 4].min() == conf.prob_thr == F(0.3), "a confidence equal to the threshold is kept, one ulp below is not"
    sent = np.sort(conf.pred[0][:, 4])[-3:]
    assert list(sent) == [np.nextafter(F(0.3), F(0)), F(0.3), np.nextafter(F(0.3), F(1))]


def test_geometry_holds_what_it_promises():
    c = pr.cases()["geometry"]
    n = c.facts["special"] + c.facts["background"]
    for b, (label, conf) in enumerate(pr.survivors(c.pred, c.prob_thr)):
        assert len(conf) == n == len(np.unique(conf))
        with np.errstate(all="ignore"):
            elem, box, _, cf = pr.filter_rows(c.pred[b], c.prob_thr)
        odd = ~np.isfinite(box).all(1)
        assert odd.sum() == 12
        rank = np.argsort(np.argsort(-cf))
        if b in (0, 3):
            assert rank[odd].max() < c.facts["special"], "non-finite boxes among the first picks"
        if b == 1:
            assert rank[odd].min() >= c.facts["background"], "non-finite boxes among the last candidates"
        assert ((box[:, 2] < 0) | (box[:, 3] < 0)).sum() >= 3 and ((box[:, 2] == 0) & (box[:, 3] == 0)).sum() == 2
    for agnostic in (False, True):
        raw, _ = pr.expected(c.id, agnostic, False)
        adj, _ = pr.expected(c.id, agnostic, True)
        for d in raw:
            assert ((d[:, 2] == 0) & (d[:, 3] == 0)).sum() == 2, "0 / 0 is not > threshold: both zero-area duplicates stay"
        assert np.isnan(raw[0]).any() and np.isinf(raw[0]).any()
        # tiny scale: everything finite ends on an edge; huge scale: everything collapses towards 0
        assert set(np.unique(adj[1][:, 0])) <= {0.0, 639.0}
        v = adj[2][:, :4]
        assert np.median(np.abs(v[np.isfinite(v)])) < 1e-35
        assert ((v != 0) & (np.abs(v) < np.finfo(F).tiny)).any(), "some quotients are subnormal"
        # the clip is std::max(lo, std::min(v, hi)), first argument on a false compare: -0.0 becomes +0.0, NaN becomes lo = 0
        with np.errstate(all="ignore"):
            _, box, _ = _picked_rows(c, 2, agnostic)
            q = box[:, 0] / F(3e38)
        assert (np.signbit(q) & (q == 0)).sum() == 1, "one picked x is -0.0 in front of the clip"
        assert not np.signbit(adj[2][:, 0]).any(), "and +0.0 behind it"
        for b in range(4):
            assert not np.isnan(adj[b][:, :4]).any() and np.isnan(raw[b][:, :4]).any(), "NaN coordinates clip to 0"
            nan_x = np.isnan(raw[b][:, 0])
            assert nan_x.any() and (adj[b][nan_x, 0] == 0).all() and (adj[b][nan_x, 2] == 0).all()
    assert list(pr.clip(np.asarray([np.nan, -0.0, -np.inf, np.inf, 5.0], F), F(0), F(639))) == [0.0, 0.0, 0.0, 639.0, 5.0]
    assert not np.signbit(pr.clip(np.asarray([-0.0], F), F(0), F(639)))[0]


def test_ties_are_decided_by_element_order_and_by_the_sign_of_zero():
    assert [cid for cid, k in pr.cases().items() if not k.distinct] == list(pr.TIE_IDS)
    c = pr.cases()["ties"]
    for b, (label, conf) in enumerate(pr.survivors(c.pred, c.prob_thr)):
        assert len(conf) == 40 and (conf == F(0.5)).all()
    rows, box, _ = _picked_rows(c, 0, False)
    assert (np.diff(rows) > 0).all() and 1 < len(rows) < 40, "picks come in element order, and the boxes do overlap"
    assert (np.diff(box[:, 0]) < 0).any(), "element order is not the order along the row"
    z = pr.cases()["ties_zero"]
    for agnostic in (False, True):
        rows, box, _ = _picked_rows(z, 0, agnostic)
        assert list(rows) == z.facts["picked_rows"] and list(box[:, 0]) == [3.0, 100.0]
    conf = z.pred[0][z.facts["rows"], 4]
    assert list(np.signbit(conf)) == [True, False, False, True] and (conf == 0).all()


# ---- the wrong intersection -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("agnostic", [False, True], ids=["perclass", "agnostic"])
def test_fmax_fmin_intersection_differs_from_the_oracle_where_the_selects_do_not(orc, agnostic):
    """inter_area with fmaxf / fminf (the kernel before this matrix) against the oracle's `a > b ? a : b`.  The two differ when the PICKED box's far edge
    x + w is NaN: the ternaries hand the NaN on, the intersection is NaN and nothing is suppressed; fminf drops it and returns a finite
    intersection.  Through the entry a picked box with a NaN edge also has a NaN area unless its width is infinite (x = -inf, w = +inf: x + w is
    NaN, the area +inf), so the quotient that decides is finite / inf = 0: the two forms part exactly where IoU 0 suppresses, at a negative
    nms_threshold.  geometry_negthr is that case; at the default threshold the same boxes give the same picks either way."""
    c = pr.cases()["geometry_negthr"]
    assert c.nms_thr < 0 and c.pred.tobytes() == pr.cases()["geometry"].pred.tobytes()
    ref = orc.yolo_postprocess(c.pred, float(c.prob_thr), float(c.nms_thr), agnostic, None)
    pr.assert_same_result(pr.expected(c.id, agnostic, False), ref, c.id)
    picks = [[len(_picked_rows(c, b, agnostic, nms=f)[0]) for b in range(4)] for f in (pr.nms, FMAX_FMIN)]
    assert picks[0] == list(ref[1])
    assert picks[1] != picks[0], "fmaxf / fminf give the oracle's picks: the case no longer separates the two forms"
    assert picks[1][0] < picks[0][0], "image 0 picks the infinite-width box early; fminf then lets it suppress finite boxes"
    g = pr.cases()["geometry"]
    for b in range(4):
        assert list(_picked_rows(g, b, agnostic, nms=FMAX_FMIN)[0]) == list(_picked_rows(g, b, agnostic)[0]), "the default threshold"


def test_rule_is_fast_enough(capsys):
    """2049 candidates take well under a second (about 0.1 s); the figure is printed, and the bar is 20 s so that only a rule that has lost its
    vectorised inner loop (minutes) can miss it, not a loaded machine"""
    import time
    c = pr.cases()["counts_2049"]
    t = time.perf_counter()
    pr.postprocess_image(c.pred[0], c.prob_thr, c.nms_thr, True)
    t = time.perf_counter() - t
    with capsys.disabled():
        print("\npost_reference rule, 2049 candidates all picked: %.3f s" % t)
    assert t < 20.0
