"""CPU: the oriented-box rule (tests/obb_reference.py) against a transcription of ultralytics' two functions in torch float64; the inputs of the
GPU file against the margin they are run under; the C-ABI of include/si_obb.h (exported, bound under its own table, absent from
include/si_hip.h and include/si_detect.h); and the stand-alone program over csrc/hip/obb_plan.h under AddressSanitizer and UBSan."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import containment as ct
import obb_reference as R
from simpleinfer_amd import _native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "si_obb.h")
HIP_DIR = os.path.join(ROOT, "simpleinfer_amd", "csrc", "hip")
ENTRIES = ["si_hip_detect_obb_postprocess_workspace_bytes", "si_hip_detect_obb_postprocess_f32"]
IOU_TOL = 1e-12           # float64: |numpy rule - torch transcription| measured at most 4.4e-16 on these inputs


# ---- ultralytics/utils/metrics.py (_get_covariance_matrix, batch_probiou) and utils/ops.py (nms_rotated), transcribed -----------------------------
def _get_covariance_matrix(boxes):
    gbbs = torch.cat((boxes[:, 2:4].pow(2) / 12, boxes[:, 4:]), dim=-1)
    a, b, c = gbbs.split(1, dim=-1)
    cos, sin = c.cos(), c.sin()
    cos2, sin2 = cos.pow(2), sin.pow(2)
    return a * cos2 + b * sin2, a * sin2 + b * cos2, (a - b) * cos * sin


def batch_probiou(obb1, obb2, eps=1e-7):
    x1, y1 = obb1[..., :2].split(1, dim=-1)
    x2, y2 = (x.squeeze(-1)[None] for x in obb2[..., :2].split(1, dim=-1))
    a1, b1, c1 = _get_covariance_matrix(obb1)
    a2, b2, c2 = (x.squeeze(-1)[None] for x in _get_covariance_matrix(obb2))
    t1 = (((a1 + a2) * (y1 - y2).pow(2) + (b1 + b2) * (x1 - x2).pow(2)) / ((a1 + a2) * (b1 + b2) - (c1 + c2).pow(2) + eps)) * 0.25
    t2 = (((c1 + c2) * (x2 - x1) * (y1 - y2)) / ((a1 + a2) * (b1 + b2) - (c1 + c2).pow(2) + eps)) * 0.5
    t3 = (((a1 + a2) * (b1 + b2) - (c1 + c2).pow(2)) / (4 * ((a1 * b1 - c1.pow(2)).clamp_(0) * (a2 * b2 - c2.pow(2)).clamp_(0)).sqrt() + eps) + eps).log() * 0.5
    bd = (t1 + t2 + t3).clamp(eps, 100.0)
    hd = (1.0 - (-bd).exp() + eps).sqrt()
    return 1 - hd


def nms_rotated(boxes, scores, threshold=0.45):
    sorted_idx = torch.argsort(scores, descending=True)
    boxes = boxes[sorted_idx]
    ious = batch_probiou(boxes, boxes).triu_(diagonal=1)
    pick = torch.nonzero(ious.max(dim=0)[0] < threshold).squeeze_(-1)
    return sorted_idx[pick]


@pytest.mark.parametrize("agnostic", [False, True])
@pytest.mark.parametrize("k", [2, 65, 257, 1025])
def test_rule_equals_the_ultralytics_transcription(k, agnostic):
    """the boxes span 60 * sqrt(k) < 2000 units, so the label * 7680 offset moves other classes out of every overlap: there the exact label
    compare and the offset agree"""
    classes = 3
    pred = R.case(5, (k,), classes)[0]
    rows, boxes, conf, label = R.candidates(pred, classes, 1, 0, 0.25)
    keep = R.keep_mask(boxes, label, 0.45, agnostic)
    tb = torch.from_numpy(boxes.astype(np.float64))
    tb[:, :2] += torch.from_numpy(label.astype(np.float64))[:, None] * (0.0 if agnostic else 7680.0)
    picks = nms_rotated(tb, torch.from_numpy(conf.astype(np.float64)))
    assert len(rows) == k and sorted(picks.tolist()) == list(np.nonzero(keep)[0]) and 0 < keep.sum() < k
    ious = batch_probiou(tb, tb).numpy()
    same = np.ones((k, k), bool) if agnostic else label[:, None] == label
    assert np.abs(ious - R.probiou(boxes))[same].max() < IOU_TOL
    # the compare the kernel makes, on the distance, decides what the compare on the IoU decides
    with np.errstate(all="ignore"):
        assert np.array_equal(R.bd_compare(R.pair_bd(boxes), 0.45), ~(R.probiou(boxes) < 0.45))


def test_gpu_inputs_hold_their_margin():
    """every seeded input of tests/test_gpu_obb.py: the fp32 restatement of the kernel's arithmetic is within DEV of float64, and no pair's
    float64 ProbIoU is within M = 8 * DEV of the threshold (the large counts are asserted where they run)"""
    import test_gpu_obb as tg
    worst = 0.0
    for count in [c for c in tg.COUNTS if c <= 257]:
        for classes in (1, 3):
            dev, gap = R.deviation_and_gap(R.case(tg.SEED, (count, 2 * count // 3 + 1), classes), classes, 1, 0, tg.PROB, tg.NMS)
            worst = max(worst, dev)
            assert dev <= tg.DEV and gap > tg.M, (count, classes, dev, gap)
    assert worst > tg.DEV / 8 and tg.M == 8 * tg.DEV, "DEV is a measurement, not a guess"


# ---- the C-ABI -----------------------------------------------------------------------------------------------------------------------------------
def test_obb_header_is_exported_and_bound(native_libs):
    H, _ = native_libs
    assert ct.header_functions(HEADER) == ENTRIES and sorted(H._si_obb_signatures) == sorted(ENTRIES)
    others = [getattr(H, n) for n in dir(H) if re.fullmatch(r"_si_\w*signatures", n) and n != "_si_obb_signatures"]
    assert len(others) >= 19 and not any(set(ENTRIES) & set(o) for o in others)
    raw = C.CDLL(_native.LIB_HIP_PATH)
    assert all(hasattr(raw, name) for name in ENTRIES)
    for other in ("si_hip.h", "si_detect.h"):
        text = open(os.path.join(ROOT, "include", other)).read()
        assert "si_hip_detect_obb" not in text and "SiDetectObb" not in text, other
    assert [n for n, _ in _native.SiDetectObbDesc._fields_] == ["n", "rows", "classes", "objectness", "extra", "layout", "ld", "image_ld", "angle_off",
                                                               "prob_threshold", "nms_threshold", "agnostic", "max_det"]
    assert C.sizeof(_native.SiDetectObbDesc) == 64 and _native.SiDetectObbDesc.image_ld.offset == 32 and C.sizeof(_native.SiDetectObbOut) == 32
    text = open(HEADER).read()
    for phrase in ("nothing is clipped", "the matrix form", "label * 7680", "!(max(bd, eps) > bd_max)", "safe inside a\n * captured graph",
                   "Refused before any device call", "Out of scope"):
        assert phrase in text, phrase


def test_obb_plan_stand_alone_under_sanitizers(tmp_path):
    exe = str(tmp_path / "test_obb_plan")
    subprocess.check_call(["g++", "-std=c++17", "-O0", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan", "-I" + HIP_DIR, os.path.join(ROOT, "tests", "cpp", "test_obb_plan.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "obb plan ok" in r.stdout and "runtime error" not in r.stderr, r.stdout[-4000:] + r.stderr[-4000:]
