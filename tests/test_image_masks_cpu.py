"""CPU: the float64 rule of the image-size masks (tests/imgmask_reference.py) against torch float64 with crop and threshold written as ultralytics
writes them, the share of pixels the bound of the GPU comparison excludes, letterbox_window against scale_masks' rounding, the C-ABI of
include/si_imgmask.h without a device, and the stand-alone program over csrc/hip/imgmask_plan.h under AddressSanitizer and UBSan."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import containment as ct
import imgmask_reference as R
from simpleinfer_amd import _native, hipops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "si_imgmask.h")
HIP_DIR = os.path.join(ROOT, "simpleinfer_amd", "csrc", "hip")
ENTRIES = ["si_hip_detect_image_masks_f32", "si_hip_detect_image_masks_kernel_name"]
BADARG, UNSUPPORTED = -1, -2
SHARED, DIRECT = "detect_image_masks_kernel<shared>", "detect_image_masks_kernel<direct>"


def crop_mask(masks, boxes):
    """ultralytics/utils/ops.py crop_mask: masks [k][h][w], boxes [k][4] xyxy"""
    _, h, w = masks.shape
    x1, y1, x2, y2 = torch.chunk(boxes[:, :, None], 4, 1)
    r = torch.arange(w, dtype=x1.dtype)[None, None, :]
    c = torch.arange(h, dtype=x1.dtype)[None, :, None]
    return masks * ((r >= x1) * (r < x2) * (c >= y1) * (c < y2))


@pytest.mark.parametrize("crop", R.CROPS)
@pytest.mark.parametrize("gname", ["identity", "x4", "offset", "down", "border"])
def test_float64_rule_equals_torch(gname, crop):
    """process_mask(upsample=True) (crop, interpolate, gt_) and process_mask_native (interpolate the scale_masks window, crop, gt_) on the
    window's float64 logits, the boxes' far edges x + w formed in fp32 as the rule forms them"""
    key = ((20, 24), 32, crop, gname, R.COUNTS[1])
    c = R.case(*key)
    ref = R.rule_f64(c.protos, c.extras, c.boxes, c.counts, c.geom, c.out_hw, crop, c.coef_off, 32, exact=True)
    x0, y0, ww, wh, out_w, out_h = (int(v) for v in c.geom[0])
    for b, (want, v, _) in enumerate(ref):
        coef = torch.from_numpy(c.extras[b, :, c.coef_off:c.coef_off + 32].astype(np.float64))
        win = torch.from_numpy(c.protos[b, y0:y0 + wh, x0:x0 + ww].astype(np.float64))
        with np.errstate(all="ignore"):
            xyxy = torch.from_numpy(np.concatenate([c.boxes[b, :, :2], c.boxes[b, :, :2] + c.boxes[b, :, 2:]], 1).astype(np.float64))
        masks = (coef @ win.reshape(-1, 32).T).view(-1, wh, ww)
        if crop == "first":
            masks = crop_mask(masks, xyxy)
        up = torch.nn.functional.interpolate(masks[None], (out_h, out_w), mode="bilinear", align_corners=False)[0]
        assert np.abs(v[:, :out_h, :out_w] - up.numpy()).max() < 1e-12
        final = (crop_mask(up, xyxy) if crop == "after" else up).gt_(0.0).numpy().astype(bool)
        away = np.abs(up.numpy()) > 1e-9
        assert np.array_equal(final[away], want[:, :out_h, :out_w].astype(bool)[away]) and 0.02 < final.mean() < 0.5
        assert not want[:, out_h:].any() and not want[:, :, out_w:].any()


def test_the_bound_excludes_under_one_percent():
    """every input of the GPU comparison against float64, with the reference alone: the float32 restatement agrees wherever the bound decides"""
    import test_gpu_image_masks as tg
    worst = 0.0
    for key in [p for p in tg.PRODUCT if p[4][0] and p[3] in ("x4", "offset", "down")]:
        ref = R.expected_f64(*key)
        decided, excluded = R.decided(ref)
        worst = max(worst, excluded)
        assert excluded <= R.EXCLUDED_CAP, (key, excluded)
        for m, (want, _, _), f32 in zip(decided, ref, R.expected(*key)):
            assert np.array_equal(want[m], f32[m]), key
    assert worst > 0, "some pixel is near zero: the bound is exercised"


@pytest.mark.parametrize("src_hw,want", [((480, 640), (0, 20, 160, 120)), ((375, 500), (0, 20, 160, 120)), ((427, 640), (0, 27, 160, 106)), ((428, 640), (0, 26, 160, 107)),
                                         ((640, 427), (27, 0, 106, 160)), ((333, 500), (0, 27, 160, 106)), ((640, 640), (0, 0, 160, 160)),
                                         ((1080, 810), (20, 0, 120, 160))])
def test_letterbox_window_rounds_as_scale_masks(src_hw, want):
    """ultralytics scale_masks on a 160 x 160 plane: top / left = int(round(pad - 0.1)), bottom / right = size - int(round(pad + 0.1)); a
    padding of 26.5 (428 rows) rounds to 26 in front and 27 behind, 26.625 and 26.72 to 27 on both sides"""
    mh = mw = 160
    gain = min(mh / src_hw[0], mw / src_hw[1])
    pad = [(mw - src_hw[1] * gain) / 2, (mh - src_hw[0] * gain) / 2]
    top, left = int(round(pad[1] - 0.1)), int(round(pad[0] - 0.1))
    bottom, right = mh - int(round(pad[1] + 0.1)), mw - int(round(pad[0] + 0.1))
    w = hipops.letterbox_window(src_hw, (mh, mw), (640, 640))
    assert tuple(w.geom) == (left, top, right - left, bottom - top, src_hw[1], src_hw[0]) and tuple(w.geom[:4]) == want
    assert w.ratio == (0.25, 0.25) and w.origin == (left, top) and R.geom_ok(w.geom, mh, mw, src_hw[0], src_hw[1])


def test_abi_without_a_device(native_libs):
    H, _ = native_libs
    assert ct.header_functions(HEADER) == ENTRIES and sorted(H._si_imgmask_signatures) == sorted(ENTRIES)
    others = [getattr(H, n) for n in dir(H) if re.fullmatch(r"_si_\w*signatures", n) and n != "_si_imgmask_signatures"]
    assert len(others) >= 20 and not any(set(ENTRIES) & set(o) for o in others)
    raw = C.CDLL(_native.LIB_HIP_PATH)
    assert all(hasattr(raw, name) for name in ENTRIES)
    for other in ("si_hip.h", "si_detect.h"):
        text = open(os.path.join(ROOT, "include", other)).read()
        assert "image_masks" not in text and "SiImageMask" not in text, other
    assert [n for n, _ in _native.SiImageMaskDesc._fields_] == ["n", "mh", "mw", "nm", "proto_ld", "max_det", "extra", "coef_off", "oh", "ow", "box_ld",
                                                               "crop", "flags"] and C.sizeof(_native.SiImageMaskDesc) == 52
    good = lambda **kw: hipops.image_mask_desc(2, 160, 160, 32, 300, 32, 640, 640, **kw)
    p = C.c_void_p(256)
    call = lambda d, ptrs=(p,) * 6: H.si_hip_detect_image_masks_f32(C.byref(d) if d is not None else None, *ptrs, None)

    def bad(**fields):
        d = good()
        for k, v in fields.items():
            setattr(d, k, v)
        return d

    # every refusal comes back before a device call: this process has no device to call
    assert call(None) == BADARG
    for i in range(6):
        assert call(good(), tuple(None if j == i else p for j in range(6))) == BADARG, i
    for i in range(5):
        assert call(good(), tuple(C.c_void_p(258) if j == i else p for j in range(6))) == BADARG, i
    for fields in (dict(n=0), dict(mh=0), dict(mw=-1), dict(nm=0), dict(extra=0), dict(oh=0), dict(ow=-5), dict(proto_ld=31), dict(box_ld=3),
                   dict(max_det=-1), dict(coef_off=-1), dict(coef_off=1), dict(crop=2), dict(crop=-1), dict(flags=2)):
        assert call(bad(**fields)) == BADARG, fields
        assert H.si_hip_detect_image_masks_kernel_name(C.byref(bad(**fields)), p, p) == b"none", fields
    for fields in (dict(nm=65, proto_ld=65, extra=65), dict(n=65536), dict(oh=65536, ow=32768), dict(mh=32768, mw=32768, proto_ld=32),
                   dict(n=65535, max_det=2 ** 31 - 1)):
        assert call(bad(**fields)) == UNSUPPORTED, fields
    assert call(bad(max_det=0)) == 0
    # the kernel name follows the arm rule (csrc/hip/imgmask_plan.h) on the nominal geometry
    name = hipops.detect_image_masks_kernel_name
    assert name(good()) == SHARED and name(good(crop="first")) == SHARED and name(good(force_direct=True)) == DIRECT
    assert name(hipops.image_mask_desc(2, 160, 160, 64, 300, 64, 640, 640)) == SHARED                 # 34 x 4 pixels of 67 floats: 36 KB
    assert name(hipops.image_mask_desc(2, 160, 160, 32, 300, 32, 160, 160)) == DIRECT                 # identity: 129 x 9 pixels do not fit
    assert name(hipops.image_mask_desc(2, 160, 160, 32, 300, 32, 40, 40)) == DIRECT                   # down-scaling shares nothing
    assert name(good(), protos_ptr=258) == "none" and name(good(), masks_ptr=0) == "none" and name(good(), masks_ptr=257) == SHARED
    text = open(HEADER).read()
    for phrase in ("bit for bit", "INSIDE", "write the image's live planes\n * as zeros", "deliberately not used", "Refused before any device call",
                   "ONE barrier", "nominal geometry"):
        assert phrase in text, phrase


def test_imgmask_plan_stand_alone_under_sanitizers(tmp_path):
    exe = str(tmp_path / "test_imgmask_plan")
    subprocess.check_call(["g++", "-std=c++17", "-O0", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan", "-I" + HIP_DIR, os.path.join(ROOT, "tests", "cpp", "test_imgmask_plan.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "imgmask plan ok" in r.stdout and "runtime error" not in r.stderr, r.stdout[-4000:] + r.stderr[-4000:]
