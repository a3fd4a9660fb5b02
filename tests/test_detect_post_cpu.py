"""CPU: the general detection post-processing rule (tests/detect_reference.py) and the host side of include/si_detect.h -- the rule in YOLOv5
mode against tests/post_reference.py on all its cases; every converted case keeps its original's survivors bit for bit and every generated
case reaches the boundary it was written for; the rule against a float64 plain-Python greedy NMS; masks_ref against a float64 einsum; the
coverage of the GPU file's matrix; the C-ABI (exported, bound under its own table, absent from include/si_hip.h, the structures' fields,
every refusal by return code without a launch, every compute entry driven by a view case of the GPU file); and the stand-alone program over
csrc/hip/detect_plan.h under AddressSanitizer and UBSan."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import containment as ct
import detect_reference as dr
import post_reference as pr
from simpleinfer_amd import _native, hipops, modelgen as mg

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "si_detect.h")
ENTRIES = ["si_hip_detect_postprocess_workspace_bytes", "si_hip_detect_postprocess_f32", "si_hip_detect_filter_kernel_name", "si_hip_detect_masks_f32",
           "si_hip_detect_masks_kernel_name"]
BADARG, UNSUPPORTED = -1, -2


# ---- the rule -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", pr.CASE_IDS)
def test_yolov5_mode_is_post_reference(cid):
    c = pr.cases()[cid]
    for agnostic in (False, True):
        for adjusted in (False, True):
            _, outs, cnt = dr.expected("v5/" + cid, agnostic, adjusted)
            pr.assert_same_result(([o.dets for o in outs], cnt), pr.expected(cid, agnostic, adjusted), cid)
    # the row index is the element index of post_reference's own filter, in its sort order
    _, outs, _ = dr.expected("v5/" + cid, False, False)
    for b, o in enumerate(outs):
        with np.errstate(all="ignore"):
            elem, box, label, conf = pr.filter_rows(c.pred[b], c.prob_thr)
            order = pr.sort_order(elem, conf)
            picks = pr.nms(box[order], label[order], c.nms_thr, False)
        assert list(o.src_rows) == list(elem[order][picks])
        pr.assert_same(o.net_boxes, box[order][picks], cid)


def _same_survivors(a, b, what):
    (e0, b0, l0, c0), (e1, b1, l1, c1) = a, b
    assert np.array_equal(e0, e1) and np.array_equal(l0, l1) and c0.tobytes() == c1.tobytes(), what
    pr.assert_same(b1, b0, what)


def test_every_conversion_keeps_the_originals_survivors():
    """... so every structural promise tests/test_postprocess_cpu.py asserts of the original holds of the conversion: the same rows survive with
    the same confidence bits, labels and box bits (v8: without the rows that have no class maximum, which a head without a box score drops at
    any finite threshold)"""
    seen = set()
    for cid, c in dr.cases().items():
        if c.origin is None:
            continue
        seen.add((cid.split("/")[0], c.origin))
        o = pr.cases()[c.origin]
        for b in range(len(c.pred)):
            with np.errstate(all="ignore"):
                want = pr.filter_rows(o.pred[b], o.prob_thr)
                got = dr.filter_rows(c.pred[b], c.desc)
            if not c.desc.objectness:
                m = want[2] >= 0
                want = tuple(v[m] for v in want)
            _same_survivors(want, got, cid)
    for kind in ("v5", "v5xy"):
        assert {o for k, o in seen if k == kind} == set(pr.CASE_IDS)
    for kind in ("v8", "v8xy"):
        assert {o for k, o in seen if k == kind} == set(pr.CASE_IDS) - set(dr.NO_V8)
    # what the excluded case would lose: its +inf box score has no counterpart (the product is +inf in every class, the label moves to 0)
    c = pr.cases()["classes"]
    with np.errstate(all="ignore"):
        want = pr.filter_rows(c.pred[0], c.prob_thr)
        got = dr.filter_rows(dr.to_noobj(c.pred)[0], dr.Desc(4, 0, 0, "cxcywh", c.prob_thr, c.nms_thr))
    assert not np.array_equal(want[2][want[2] >= 0], got[2])


def test_generated_cases_reach_their_boundaries():
    cs = dr.cases()
    c = cs["v8_classes"]
    for b in range(2):
        with np.errstate(all="ignore"):
            elem, box, label, conf = dr.filter_rows(c.pred[b], c.desc)
        assert len(conf) == len(c.facts["special_labels"]) + c.facts["background"] and (label >= 0).all(), "rows without a maximum are dropped"
        assert np.isposinf(conf.max()) and conf.min() == F(0.25), "+inf first; a confidence equal to the threshold is kept"
    for agnostic in (False, True):
        _, outs, _ = dr.expected("v8_classes", agnostic)
        for o in outs:
            assert np.isposinf(o.dets[0, 4]) and o.dets[0, 5] == 3
    with np.errstate(all="ignore"):
        _, _, label, _ = dr.filter_rows(np.asarray([[0, 0, 1, 1, 0.5, 0.9, 0.9, 0.3], [0, 0, 1, 1, 0.9, 0.9, 0.9, 0.9], [0, 0, 1, 1] + [np.nan] * 4], F),
                                        dr.Desc(4, 0, 0, "cxcywh", F(-np.inf)))
    assert list(label) == [1, 0, -1], "tied maxima: the first wins; no maximum: label -1"
    m = cs["v8_minus_one"]
    assert np.isneginf(m.desc.prob_thr)
    for b in range(2):
        with np.errstate(all="ignore"):
            elem, box, label, conf = dr.filter_rows(m.pred[b], m.desc)
        assert len(elem) == m.pred.shape[1] == 101 and (label == -1).sum() == 3 and (conf[label == -1] == -pr.FLT_MAX).all()
    for agnostic in (False, True):
        _, outs, _ = dr.expected("v8_minus_one", agnostic)
        for o in outs:
            minus = o.dets[o.dets[:, 5] == -1]
            assert len(minus) == 2 and (minus[:, 4] == -pr.FLT_MAX).all(), "two of the three rows without a maximum share a box: the later one goes"
    for rows in (1, 127, 128, 129, 257):
        c = cs["sized_rows%d" % rows]
        assert c.pred.shape[1] == rows
        for b in range(2):
            assert len(dr.filter_rows(c.pred[b], c.desc)[0]) == min(rows, 33)
    for cid in ("sized_none", "sized_none_v5"):
        _, outs, cnt = dr.expected(cid)
        assert list(cnt) == [0, 0] and all(len(dr.filter_rows(p, cs[cid].desc)[0]) == 0 for p in cs[cid].pred)
    assert cs["sized_lvis"].desc.ne + 32 == 1300 and cs["sized_ne128"].desc.ne + 32 == 128
    for cid in ("sized_lvis", "sized_ne128"):
        _, outs, cnt = dr.expected(cid, False, False, 32)
        assert all(1 < k < 70 for k in cnt), "real suppression"
        assert max(int(o.dets[:, 5].max()) for o in outs) >= cs[cid].desc.classes - 5, "labels up to the last classes"


def test_the_gpu_matrix_covers_every_listed_value():
    import test_gpu_detect_post as tg
    cells = tg.MATRIX
    cs = dr.cases()
    assert len(cells) < 150, "thinned: the file stays within seconds"
    assert {m.layout for m in cells} == {"rows", "channels"} and {m.extra for m in cells} == {0, 1, 32, 51} == set(tg.EXTRAS)
    assert {cs[m.cid].desc.box_format for m in cells} == {"cxcywh", "xyxy"} and {cs[m.cid].desc.objectness for m in cells} == {0, 1}
    assert {m.agnostic for m in cells} == {False, True} and {m.adjusted for m in cells} == {False, True}
    for layout in ("rows", "channels"):
        sub = [m for m in cells if m.layout == layout]
        assert {m.extra for m in sub} == {0, 1, 32, 51}, layout
        assert {(cs[m.cid].desc.box_format, cs[m.cid].desc.objectness) for m in sub} == {("cxcywh", 0), ("cxcywh", 1), ("xyxy", 0), ("xyxy", 1)}, layout
        assert {1, 127, 128, 129, 257} <= {cs[m.cid].pred.shape[1] for m in sub}, layout
        assert {1, 2, 63, 64, 65, 80} <= {cs[m.cid].desc.classes for m in sub}, layout
        assert {m.agnostic for m in sub} == {False, True}
    survivors = set()
    for m in cells:
        c = cs[m.cid]
        with np.errstate(all="ignore"):
            survivors |= {len(dr.filter_rows(p, c.desc)[0]) for p in c.pred}
    assert {0, 1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025} <= survivors
    ne = {(m.layout, cs[m.cid].desc.ne + m.extra) for m in cells}
    assert ("rows", 128) in ne and ("channels", 1300) in ne and max(e for lay, e in ne if lay == "rows") == 128
    assert {m.cid for m in cells} == {cid for cid in cs if not cid.startswith("v5/")}, "every case that is not the old entry's own (those run old against new)"


def _nms64(boxes, labels, thr, agnostic):
    """a plain-Python greedy NMS in float64: no selects, no vector tricks"""
    picks = []
    for i, (x, y, w, h) in enumerate(boxes):
        ok = True
        for j in picks:
            X, Y, W, H = boxes[j]
            iw, ih = min(x + w, X + W) - max(x, X), min(y + h, Y + H) - max(y, Y)
            inter = iw * ih if iw > 0 and ih > 0 else 0.0
            if (agnostic or labels[i] == labels[j]) and inter / (w * h + W * H - inter) > thr:
                ok = False
        if ok:
            picks.append(i)
    return picks


@pytest.mark.parametrize("box_format", ["cxcywh", "xyxy"])
@pytest.mark.parametrize("objectness", [0, 1])
def test_rule_equals_a_float64_restatement_on_well_separated_data(objectness, box_format):
    """confidences 2^-10 apart and IoUs at least 1e-5 away from the threshold: float64 and fp32 take the same decisions"""
    r = np.random.Generator(np.random.Philox(77 + objectness))
    rows, nc, k = 300, 6, 120
    for trial in range(3):
        boxes = np.concatenate([r.uniform(0, 160, (k, 2)), r.uniform(20, 70, (k, 2))], 1).round(2)
        conf = (0.3 + 2.0 ** -10 * r.permutation(k)).astype(F)
        label = r.integers(0, nc, k)
        pred = pr._embed(pr._rows(boxes, conf, label, nc, r), rows, r)[None]
        if box_format == "xyxy":
            pred = dr.to_xyxy(pred)
        if not objectness:
            pred = dr.to_noobj(pred)
        pred = dr.with_payload(pred, 3, seed=trial)
        for agnostic in (False, True):
            desc = dr.Desc(nc, objectness, 3, box_format, F(0.25), F(0.45), agnostic)
            (got,), _ = dr.postprocess(pred, desc)
            p = pred[0].astype(np.float64)
            first = 4 + objectness
            best = p[:, first:first + nc].max(1)
            c64 = p[:, 4] * best if objectness else best
            keep = np.nonzero(c64 >= 0.25)[0]
            keep = keep[np.argsort(-c64[keep], kind="stable")]
            b = p[keep, :4]
            b64 = np.stack([b[:, 0] - b[:, 2] / 2, b[:, 1] - b[:, 3] / 2, b[:, 2], b[:, 3]], 1) if box_format == "cxcywh" else np.stack(
                [b[:, 0], b[:, 1], b[:, 2] - b[:, 0], b[:, 3] - b[:, 1]], 1)
            lab = p[keep, first:first + nc].argmax(1)
            # the margin that makes float64 decisive: no IoU within 1e-5 of the threshold.  The fp32 quotient is a dozen operations on boxes that
            # carry 2^-24 relative each: its error stays below 1e-6
            x, y, w, h = b64.T
            iw = np.minimum(x[:, None] + w[:, None], x + w) - np.maximum(x[:, None], x)
            ih = np.minimum(y[:, None] + h[:, None], y + h) - np.maximum(y[:, None], y)
            inter = np.where((iw > 0) & (ih > 0), iw * ih, 0.0)
            assert np.abs(inter / (w[:, None] * h[:, None] + w * h - inter) - 0.45).min() > 1e-5
            picks = _nms64([tuple(v) for v in b64], list(lab), 0.45, agnostic)
            assert len(keep) == k and list(got.src_rows) == [int(keep[i]) for i in picks], (trial, agnostic)
            assert np.abs(got.net_boxes - b64[picks]).max() < 1e-4 and list(got.dets[:, 5]) == [float(lab[i]) for i in picks]
            assert got.extras.tobytes() == pred[0][got.src_rows, -3:].tobytes()


# ---- masks ----------------------------------------------------------------------------------------------------------------------------------
def test_masks_ref_equals_a_float64_einsum_outside_the_margin():
    """wherever |dot64| exceeds 1e-3 of sum |c_k p_k| the fp32 index-order dot has the float64 dot's sign (32 roundings of 2^-24 are far
    below that); at most 1 % of the in-box pixels may fall under the margin -- a condition on the generator, asserted here"""
    under = inbox = 0
    for cid, c in dr.mask_cases().items():
        if c.protos.shape[1] * c.protos.shape[2] > 1000:
            continue
        ref = dr.mask_expected(cid)
        p64, e64 = c.protos.astype(np.float64), c.extras.astype(np.float64)
        nm = c.protos.shape[3]
        for b, planes in enumerate(ref):
            for d in range(len(planes)):
                coef = e64[b, d, c.coef_off:c.coef_off + nm]
                dot = np.einsum("hwk,k->hw", p64[b], coef)
                mag = np.einsum("hwk,k->hw", np.abs(p64[b]), np.abs(coef))
                bx, by, bw, bh = (float(v) for v in c.net_boxes[b, d])
                with np.errstate(all="ignore"):
                    cc, rr = np.arange(c.protos.shape[2])[None, :], np.arange(c.protos.shape[1])[:, None]
                    rw, rh = float(c.ratio_w), float(c.ratio_h)
                    crop = (cc >= F(bx) * F(rw)) & (cc < (F(bx) + F(bw)) * F(rw)) & (rr >= F(by) * F(rh)) & (rr < (F(by) + F(bh)) * F(rh))
                # (products that underflow are outside the argument: the exact-zero and subnormal dots are pinned by the test below)
                sure = (np.abs(dot) > 1e-3 * mag) & (mag > 1e-30)
                assert np.array_equal(planes[d][sure], (crop & (dot > 0))[sure].astype(np.uint8)), (cid, b, d)
                assert not planes[d][~crop].any(), "nothing is set outside the crop"
                under += int((crop & ~sure).sum())
                inbox += int(crop.sum())
    assert inbox > 5000 and under <= 0.01 * inbox, (under, inbox)


def test_mask_cases_hold_what_they_promise():
    cs = dr.mask_cases()
    assert {(c.protos.shape[1], c.protos.shape[2]) for c in cs.values()} >= set(dr.MASK_SIZES) | {(160, 160)}
    assert {c.protos.shape[3] for c in cs.values()} == set(dr.MASK_NM)
    for (mh, mw) in dr.MASK_SIZES:
        for nm in dr.MASK_NM:
            c = cs["m%dx%d_nm%d" % (mh, mw, nm)]
            max_det = c.extras.shape[1]
            assert list(c.counts) == [0, 1, max_det, max_det + 5]
    # edges exactly on integers: pixel c == x1 is kept, pixel c == x2 is not
    crop = dr.mask_crop(dr.mask_boxes(20, 24, 0.25, 0.25, None, 13)[12], 20, 24, 0.25, 0.25)
    assert crop[1:3, 1:3].all() and crop.sum() == 4 and not crop[3].any() and not crop[:, 3].any() and not crop[0].any()
    # empty, inverted, NaN and outside boxes give empty crops
    boxes = dr.mask_boxes(20, 24, 0.25, 0.25, None, 14)
    for i in (6, 7, 8, 9, 10, 11):
        assert not dr.mask_crop(boxes[i], 20, 24, 0.25, 0.25).any(), i
    assert dr.mask_crop(boxes[13], 20, 24, 0.25, 0.25).all() and 0 < dr.mask_crop(boxes[1], 20, 24, 0.25, 0.25).sum() < 480
    # dots exactly 0 and the smallest subnormal either side: detections 0..2 read prototype 0 with coefficients 1, -1, 0.5
    c = cs["m5x7_nm32"]
    ref = dr.mask_expected("m5x7_nm32")
    assert list(c.protos[2, 0, :4, 0]) == [0.0, dr.SUB, -dr.SUB, 0.0] and np.signbit(c.protos[2, 0, 3, 0])
    assert list(ref[2][0][0, :4]) == [0, 1, 0, 0] and list(ref[2][1][0, :4]) == [0, 0, 1, 0], "1 * SUB > 0; -1 * -SUB > 0; 0 and -0 are not"
    assert list(ref[2][2][0, :4]) == [0, 0, 0, 0], "0.5 * SUB rounds to 0 (ties to even): a dot of exactly 0 from a non-zero product"
    assert dr.mask_dots(c.protos[2], c.extras[2, 2, c.coef_off:c.coef_off + 32])[0, 1] == 0


# ---- the toy --------------------------------------------------------------------------------------------------------------------------------
def test_toy_yolov8_seg_has_two_outputs():
    from ct_reference import _parse
    for channels_first in (True, False):
        b = mg.build_toy_yolov8_seg(2, 64, 5, 32, channels_first)
        types = [_parse(ln)[0] for ln in b.lines]
        assert types[-4:] == ["nn.Conv2d", "nn.ReLU", "nn.Conv2d", "pnnx.Output"] and types.count("pnnx.Output") == 2
        assert ("Tensor.permute" in types) == (not channels_first)
        outs = [_parse(ln)[2][0] for ln in b.lines if ln.startswith("pnnx.Output")]
        assert [b.shapes[o] for o in outs] == [(2, 41, 320) if channels_first else (2, 320, 41), (2, 32, 16, 16)]


# ---- the C-ABI ------------------------------------------------------------------------------------------------------------------------------
def _struct_fields(name):
    m = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), open(HEADER).read(), flags=re.S)
    body = re.sub(r"/\*.*?\*/", " ", m.group(1), flags=re.S)
    out = []
    for typ, names in re.findall(r"\b(int\s*\*|float\s*\*|long long|int|float)\s+([^;]+);", body):
        out += [(n.strip(), typ.replace(" ", "")) for n in names.split(",")]
    return out


def test_detect_header_is_exported_and_bound(native_libs):
    H, _ = native_libs
    declared = ct.header_functions(HEADER)
    assert declared == ENTRIES
    assert sorted(H._si_detect_signatures) == sorted(declared)
    others = [getattr(H, n) for n in dir(H) if re.fullmatch(r"_si_\w*signatures", n) and n != "_si_detect_signatures"]
    assert len(others) >= 18 and not any(set(declared) & set(o) for o in others)
    raw = C.CDLL(_native.LIB_HIP_PATH)
    assert not [name for name in declared if not hasattr(raw, name)]
    ctypes_of = {"int": C.c_int, "longlong": C.c_longlong, "float": C.c_float, "int*": C.c_void_p, "float*": C.c_void_p}
    for name, cls in (("SiDetectPostDesc", _native.SiDetectPostDesc), ("SiDetectPostOut", _native.SiDetectPostOut), ("SiDetectMaskDesc", _native.SiDetectMaskDesc)):
        assert [(n, ctypes_of[t]) for n, t in _struct_fields(name)] == list(cls._fields_), name
    assert [n for n, _ in _native.SiDetectPostDesc._fields_] == ["n", "rows", "classes", "objectness", "extra", "layout", "ld", "image_ld", "box_format",
                                                                "prob_threshold", "nms_threshold", "agnostic", "max_det"]
    assert C.sizeof(_native.SiDetectPostDesc) == 64 and _native.SiDetectPostDesc.image_ld.offset == 32 and _native.SiDetectPostDesc.max_det.offset == 56
    assert C.sizeof(_native.SiDetectPostOut) == 40 and C.sizeof(_native.SiDetectMaskDesc) == 40
    text = open(HEADER).read()
    for phrase in ("first-maximum class score", "x1 - x0, y1 - y0", "the payload is read for\n * the stored detections alone", "safe inside a captured graph",
                   "No host round trip", "a NaN keeps its bits", "The\n * matrix cores are not used", "Refused before any device call"):
        assert phrase in text, phrase


def test_si_hip_header_declares_none_of_them():
    text = open(ct.HEADER).read()
    for name in ENTRIES + ["SiDetectPostDesc", "SiDetectPostOut", "SiDetectMaskDesc", "si_hip_detect"]:
        assert name not in text, name


def test_every_compute_entry_of_the_detect_header_is_driven():
    """the rule of tests/test_containment_cpu.py for include/si_hip.h, applied to include/si_detect.h and the view cases of the GPU file"""
    import test_gpu_detect_post as tg
    entries = [n for n in ct.header_functions(HEADER) if not ct.is_exempt(n)]
    assert entries == ["si_hip_detect_postprocess_f32", "si_hip_detect_masks_f32"]
    driven = {e for v in tg.VIEW_CASES for e in v.entries}
    assert set(entries) <= driven and driven <= set(ct.header_functions(HEADER))
    # both layouts with ld and image_ld gaps and a base pointer off by one element; both mask forms with gaps
    post = [v for v in tg.VIEW_CASES if v.layout]
    assert {v.layout for v in post} == {"rows", "channels"}
    for layout in ("rows", "channels"):
        assert any(v.layout == layout and v.ld_pad and v.image_pad and v.off == 1 for v in post), layout
    masks = [v for v in tg.VIEW_CASES if not v.layout]
    assert any(v.off == 1 for v in masks) and any(v.off == 0 and v.ld_pad % 4 == 0 and dr.mask_cases()[v.cid].protos.shape[3] == 32 for v in masks)


def test_the_plan_header_needs_no_device():
    hip_dir = os.path.join(ROOT, "simpleinfer_amd", "csrc", "hip")
    for src in ("postprocess.hip", "detect_masks.hip"):
        text = open(os.path.join(hip_dir, src)).read()
        assert '#include "detect_plan.h"' in text and "hipMalloc" not in text and "hipStreamSynchronize" not in text and "hipDeviceSynchronize" not in text
    plan = re.sub(r"//[^\n]*", "", open(os.path.join(hip_dir, "detect_plan.h")).read())
    assert "hip" not in plan.lower() and set(re.findall(r"#include\s+[<\"]([^>\"]+)[>\"]", plan)) == {"cstdint", "cstddef"}


def test_abi_refusals_without_a_launch(native_libs):
    """every refusal happens before any device call: the addresses are made up"""
    H, _ = native_libs
    P, A, D, N, W, X, Y, Z = (C.c_void_p((j + 1) << 24) for j in range(8))

    def out(dets=D, counts=N, src_rows=X, net_boxes=Y, extras=Z):
        return _native.SiDetectPostOut(*[p.value if p is not None else None for p in (dets, counts, src_rows, net_boxes, extras)])

    def desc(n=2, rows=300, classes=80, **kw):
        return hipops.detect_desc(n, rows, classes, **kw)

    def call(d, pred=P, o=None, ws=W, ws_bytes=None):
        o = out() if o is None else o
        need = H.si_hip_detect_postprocess_workspace_bytes(C.byref(d))
        return H.si_hip_detect_postprocess_f32(C.byref(d), pred, A, C.byref(o), ws, need if ws_bytes is None else ws_bytes, None)

    def name(d, pred=P):
        return H.si_hip_detect_filter_kernel_name(C.byref(d), pred)

    def refused(d, code, what=""):
        assert call(d, ws_bytes=1 << 40) == code, (what, call(d, ws_bytes=1 << 40))
        assert name(d) == b"none" and H.si_hip_detect_postprocess_workspace_bytes(C.byref(d)) == 0, what

    assert name(desc()) == b"detect_filter_rows_kernel" and name(desc(layout="channels")) == b"detect_filter_channels_kernel"
    assert name(desc(extra=32, objectness=True, box_format="xyxy")) == b"detect_filter_rows_kernel"
    assert name(desc(classes=1264, extra=32, layout="channels")) == b"detect_filter_channels_kernel"
    # the workspace: the YOLOv5 entry's bytes and two more row arrays
    old = H.si_hip_yolo_postprocess_workspace_bytes(2, 300, 85)
    new = H.si_hip_detect_postprocess_workspace_bytes(C.byref(desc(objectness=True)))
    assert new == old + 2 * ((2 * 300 * 4 + 255) // 256 * 256)
    assert old == 62720, "the byte count of si_hip_yolo_postprocess_workspace_bytes(2, 300, 85) is what it was before this header existed"
    # null pointers
    assert H.si_hip_detect_postprocess_f32(None, P, A, C.byref(out()), W, 1 << 30, None) == BADARG
    assert H.si_hip_detect_postprocess_f32(C.byref(desc()), P, A, None, W, 1 << 30, None) == BADARG
    assert call(desc(), pred=None) == BADARG and call(desc(), ws=None) == BADARG and call(desc(), o=out(counts=None)) == BADARG
    assert call(desc(), o=out(dets=None)) == BADARG
    assert H.si_hip_detect_filter_kernel_name(None, P) == b"none" and name(desc(), None) == b"none" and H.si_hip_detect_postprocess_workspace_bytes(None) == 0
    assert call(desc(), ws_bytes=new - 1) == BADARG, "a workspace too small"
    assert call(desc(), pred=C.c_void_p(P.value + 2)) == BADARG and name(desc(), C.c_void_p(P.value + 2)) == b"none", "a pointer off its element"
    # sizes, enums, strides
    for field in ("n", "rows", "classes", "ld"):
        for value in (0, -1):
            d = desc()
            setattr(d, field, value)
            refused(d, BADARG, (field, value))
    for field, value in (("extra", -1), ("max_det", -1), ("objectness", 2), ("objectness", -1), ("layout", 2), ("layout", -1), ("box_format", 2),
                         ("box_format", -1), ("image_ld", -1), ("ld", 83), ("image_ld", 299 * 84 + 83)):
        d = desc()
        setattr(d, field, value)
        refused(d, BADARG, (field, value))
    d = desc(layout="channels")
    d.ld = 299
    refused(d, BADARG, "channels: ld < rows")
    d = desc(layout="channels")
    d.image_ld = 83 * 300 + 299
    refused(d, BADARG, "channels: images interleave")
    # unsupported: the grid, the staged form's limit, the index types
    refused(desc(n=65536, rows=4), UNSUPPORTED, "n beyond a grid's y")
    assert name(desc(n=65535, rows=4)) != b"none"
    refused(desc(classes=124, objectness=True), UNSUPPORTED, "ROWS with ne = 129")
    refused(desc(classes=92, extra=33), UNSUPPORTED, "ROWS with ne = 129 through the payload")
    assert name(desc(classes=123, objectness=True)) == b"detect_filter_rows_kernel" and name(desc(classes=124, objectness=True, layout="channels")) != b"none"
    refused(desc(rows=1 << 28, classes=4), UNSUPPORTED, "an image beyond 31 bits")
    refused(desc(rows=1 << 28, classes=4, layout="channels"), UNSUPPORTED, "an image beyond 31 bits")
    refused(desc(n=65535, rows=1 << 20, classes=4, image_ld=1 << 31), UNSUPPORTED, "2^47 elements across the images")
    # max_det = 0: dets may be null
    assert H.si_hip_detect_postprocess_workspace_bytes(C.byref(desc(max_det=0))) > 0 and name(desc(max_det=0)) != b"none"

    # ---- masks
    M = C.c_void_p(9 << 24)

    def mdesc(n=2, mh=160, mw=160, nm=32, max_det=300, extra=32, **kw):
        return hipops.detect_mask_desc(n, mh, mw, nm, max_det, extra, **kw)

    def mcall(d, protos=P, extras=Z, boxes=Y, counts=N, masks=M):
        return H.si_hip_detect_masks_f32(C.byref(d), protos, extras, boxes, counts, masks, None)

    def mname(d, protos=P):
        return H.si_hip_detect_masks_kernel_name(C.byref(d), protos)

    assert mname(mdesc()) == b"detect_masks_kernel<32>" and mname(mdesc(proto_ld=36)) == b"detect_masks_kernel<32>"
    assert mname(mdesc(proto_ld=33)) == b"detect_masks_kernel<0>" and mname(mdesc(), C.c_void_p(P.value + 4)) == b"detect_masks_kernel<0>"
    assert mname(mdesc(nm=1, extra=51, coef_off=50)) == b"detect_masks_kernel<0>" and mname(mdesc(nm=64, extra=64)) == b"detect_masks_kernel<0>"
    assert H.si_hip_detect_masks_f32(None, P, Z, Y, N, M, None) == BADARG and H.si_hip_detect_masks_kernel_name(None, P) == b"none"
    for k in ("protos", "extras", "boxes", "counts", "masks"):
        assert mcall(mdesc(), **{k: None}) == BADARG, k
    assert mname(mdesc(), None) == b"none" and mname(mdesc(), C.c_void_p(P.value + 1)) == b"none" and mcall(mdesc(), protos=C.c_void_p(P.value + 1)) == BADARG
    for field in ("n", "mh", "mw", "nm", "extra"):
        for value in (0, -1):
            d = mdesc()
            setattr(d, field, value)
            assert mcall(d) == BADARG and mname(d) == b"none", (field, value)
    for field, value in (("proto_ld", 31), ("max_det", -1), ("coef_off", -1), ("coef_off", 1)):
        d = mdesc()
        setattr(d, field, value)
        assert mcall(d) == BADARG and mname(d) == b"none", (field, value)
    for d, what in ((mdesc(nm=65, extra=65), "nm 65"), (mdesc(n=65536), "n"), (mdesc(mh=8192, mw=8192), "prototypes beyond 31 bits"),
                    (mdesc(n=65535, mh=4096, mw=4096, max_det=1 << 20), "mask bytes beyond 2^46")):
        assert mcall(d) == UNSUPPORTED and mname(d) == b"none", what


# ---- the plan arithmetic ----------------------------------------------------------------------------------------------------------------------
SANITIZE = ["-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"]      # the runtimes inside the program: it starts the same under any environment


def test_plan_arithmetic_stand_alone_under_sanitizers(tmp_path):
    exe = str(tmp_path / "test_detect_plan")
    subprocess.check_call(["g++", "-std=c++17", "-O0", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined"] + SANITIZE +
                          ["-I" + os.path.join(ROOT, "simpleinfer_amd", "csrc", "hip"), os.path.join(ROOT, "tests", "cpp", "test_detect_plan.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "detect plan ok" in r.stdout and "runtime error" not in r.stderr, r.stdout[-4000:] + r.stderr[-4000:]
