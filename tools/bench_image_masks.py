"""tools/bench_image_masks.py -- time of si_hip_detect_image_masks_f32 (include/si_imgmask.h).  Run on the GPU.

The workload of a 640 x 640 `-seg` export at batch 32: prototypes 32 x 160 x 160 x 32, masks 32 x 20 x 640 x 640 bytes, 20 live detections per
image with boxes of mixed size, both crops.  Beside it, in the same process and window by window in turn: a device fill of the same output bytes
(the floor: once the logits are shared the kernel is bound by its stores) and si_hip_detect_masks_f32 on the same inputs (the 160 x 160 planes,
for scale).  Windows of back-to-back calls between two device events after a warm-up; the median window of each and the share of (tile,
detection) pairs that took the zero path.  Every number is a time on the device ended by an event; nothing here asserts a speed."""
import argparse
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from simpleinfer_amd import _native, hipops  # noqa: E402
from up_reference import axis_step, axis_taps  # noqa: E402
from bench_detect_post import Timer, stats  # noqa: E402

N, MH, MW, NM, OH, OW, DETS = 32, 160, 160, 32, 640, 640, 20
TILE_W, TILE_H = 128, 8     # csrc/hip/imgmask_plan.h


def boxes_of(r, w, h):
    """[N][DETS][4] {x, y, w, h} in a w x h frame: sides between 5 % and 60 % of the frame, some across the border"""
    bw, bh = r.uniform(0.05, 0.6, (N, DETS)) * w, r.uniform(0.05, 0.6, (N, DETS)) * h
    x, y = r.uniform(-0.05, 0.95, (N, DETS)) * w - bw * 0.2, r.uniform(-0.05, 0.95, (N, DETS)) * h - bh * 0.2
    return np.stack([x, y, bw, bh], -1).astype(np.float32)


def zero_share(boxes, first):
    """share of (tile, detection) pairs whose tile the box (crop after) or whose footprint the box (crop first) does not meet: the kernel's test"""
    x1, y1, x2, y2 = boxes[..., 0], boxes[..., 1], boxes[..., 0] + boxes[..., 2], boxes[..., 1] + boxes[..., 3]
    tx0, ty0 = np.arange(0, OW, TILE_W), np.arange(0, OH, TILE_H)
    tx1, ty1 = np.minimum(tx0 + TILE_W, OW) - 1, np.minimum(ty0 + TILE_H, OH) - 1
    if first:
        cx0, cx1, _, _ = axis_taps(MW, OW, axis_step("bilinear", MW, OW), False)
        cy0, cy1, _, _ = axis_taps(MH, OH, axis_step("bilinear", MH, OH), False)
        tx0, tx1, ty0, ty1 = cx0[tx0], cx1[tx1], cy0[ty0], cy1[ty1]
    mx = (tx1[None, None, :] >= x1[..., None]) & (tx0[None, None, :] < x2[..., None])
    my = (ty1[None, None, :] >= y1[..., None]) & (ty0[None, None, :] < y2[..., None])
    return 1.0 - float((mx[:, :, None, :] & my[:, :, :, None]).mean())


def main(windows, calls, out_path):
    H = _native.hip()
    r = np.random.Generator(np.random.Philox(77))
    protos = hipops.DeviceBuffer.from_numpy(r.uniform(-1, 1, (N, MH, MW, NM)).astype(np.float32))
    extras = hipops.DeviceBuffer.from_numpy(r.uniform(-1, 1, (N, DETS, NM)).astype(np.float32))
    counts = hipops.DeviceBuffer.from_numpy(np.full(N, DETS, np.int32))
    geom = hipops.DeviceBuffer.from_numpy(np.tile(np.asarray([0, 0, MW, MH, OW, OH], np.int32), (N, 1)))
    masks, low = hipops.DeviceBuffer(N * DETS * OH * OW), hipops.DeviceBuffer(N * DETS * MH * MW)
    host = {"after": boxes_of(r, OW, OH), "first": boxes_of(r, MW, MH)}
    dev = {k: hipops.DeviceBuffer.from_numpy(v) for k, v in host.items()}
    net = hipops.DeviceBuffer.from_numpy(host["after"])           # network-frame boxes for detect_masks: the 640 x 640 frame
    desc = {k: hipops.image_mask_desc(N, MH, MW, NM, DETS, NM, OH, OW, crop=k) for k in host}
    dlow = hipops.detect_mask_desc(N, MH, MW, NM, DETS, NM)

    def image(k):
        def call():
            rc = H.si_hip_detect_image_masks_f32(C.byref(desc[k]), protos.ptr, extras.ptr, dev[k].ptr, counts.ptr, geom.ptr, masks.ptr, None)
            assert rc == 0, rc
        return call

    def fill():
        rc = H.si_hip_memset_async(masks.ptr, 0, masks.nbytes, None)
        assert rc == 0, rc

    def lowres():
        rc = H.si_hip_detect_masks_f32(C.byref(dlow), protos.ptr, extras.ptr, net.ptr, counts.ptr, low.ptr, None)
        assert rc == 0, rc

    runs = {"fill of the output bytes (floor)": fill, "detect_masks 160 x 160 (scale)": lowres, "image masks, crop after": image("after"),
            "image masks, crop first": image("first")}
    t = Timer()
    for f in runs.values():
        t.window(f, 3)
    times = {k: [] for k in runs}
    for _ in range(windows):
        for k, f in runs.items():
            times[k].append(t.window(f, calls))
    lines = ["image masks: %d x %d x %d x %d prototypes -> %d x %d x %d x %d bytes (%.1f MB), kernels %s / %s; %d windows of %d calls, interleaved" % (
        N, MH, MW, NM, N, DETS, OH, OW, masks.nbytes / 1e6, hipops.detect_image_masks_kernel_name(desc["after"], protos.ptr, masks.ptr),
        hipops.detect_image_masks_kernel_name(desc["first"], protos.ptr, masks.ptr), windows, calls)]
    floor = float(np.median(times["fill of the output bytes (floor)"]))
    for k, v in times.items():
        lines.append("    %-34s %s  %.2f x the fill, %.0f GB/s of output" % (k, stats(v), np.median(v) / floor,
                                                                            (low.nbytes if "160" in k else masks.nbytes) / np.median(v) / 1e6))
    lines.append("    (tile, detection) pairs on the zero path: %.1f %% (crop after), %.1f %% (crop first); the direct arm is not measured here" % (
        100 * zero_share(host["after"], False), 100 * zero_share(host["first"], True)))
    print("\n".join(lines))
    if out_path:
        with open(out_path, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=21)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--out", default="", help="append the lines to this file as well")
    a = ap.parse_args()
    main(a.windows, a.calls, a.out)
