"""tools/bench_obb.py -- time of si_hip_detect_obb_postprocess_f32 (include/si_obb.h).  Run on the GPU.

The shape of a 1024 x 1024 `-obb` export: 32 images x 21504 rows x (4 + 15 classes + 1 angle).  Two candidate counts: `realistic` (a few hundred
rows per image above the threshold) and `all` (every row above it: the triangular pass at its full 21504 x 21504 / 2 pairs per image).  The
yardstick is si_hip_detect_postprocess_f32 -- the axis-aligned rule -- on the same rows with the angle riding as payload.  Windows of
back-to-back calls between two device events, the two entries alternating window by window in one process; the median window of each and the
spread of the yardstick's windows.  Every number is a time on the device ended by an event; nothing here asserts a speed."""
import argparse
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from simpleinfer_amd import _native, hipops  # noqa: E402
from obb_reference import make_boxes  # noqa: E402
from bench_detect_post import Timer, stats  # noqa: E402

N, ROWS, CLASSES = 32, 21504, 15


def predictions(seed, candidates):
    """[N][ROWS][20]: `candidates` rows per image with a confidence in [0.3, 0.9), the others below 0.2; boxes at a constant density"""
    r = np.random.Generator(np.random.Philox(seed))
    pred = np.zeros((N, ROWS, 4 + CLASSES + 1), np.float32)
    for b in range(N):
        boxes = make_boxes(seed * 1000 + b, ROWS)
        conf = r.uniform(0.01, 0.2, ROWS).astype(np.float32)
        hot = r.permutation(ROWS)[:candidates]
        conf[hot] = r.uniform(0.3, 0.9, candidates).astype(np.float32)
        pred[b, :, :4] = boxes[:, :4]
        pred[b, np.arange(ROWS), 4 + r.integers(0, CLASSES, ROWS)] = conf
        pred[b, :, -1] = boxes[:, 4]
    return pred


def entries(pred, max_det=300):
    H = _native.hip()
    dpred = hipops.DeviceBuffer.from_numpy(pred)
    do = hipops.detect_obb_desc(N, ROWS, CLASSES, 1, 0, max_det=max_det)
    dp = hipops.detect_desc(N, ROWS, CLASSES, False, 1, max_det=max_det)
    wo, wp = hipops.DeviceBuffer(hipops.detect_obb_workspace_bytes(do)), hipops.DeviceBuffer(hipops.detect_workspace_bytes(dp))
    obbs, dets, rows_, extras = (hipops.DeviceBuffer(N * max_det * k * 4) for k in (7, 6, 1, 1))
    co, cp = hipops.DeviceBuffer(N * 4), hipops.DeviceBuffer(N * 4)
    oo = _native.SiDetectObbOut(obbs.ptr, co.ptr, rows_.ptr, extras.ptr)
    po = _native.SiDetectPostOut(dets.ptr, cp.ptr, rows_.ptr, None, extras.ptr)

    def obb():
        rc = H.si_hip_detect_obb_postprocess_f32(C.byref(do), dpred.ptr, None, C.byref(oo), wo.ptr, wo.nbytes, None)
        assert rc == 0, rc

    def plain():
        rc = H.si_hip_detect_postprocess_f32(C.byref(dp), dpred.ptr, None, C.byref(po), wp.ptr, wp.nbytes, None)
        assert rc == 0, rc

    return obb, plain, co, cp, (dpred, wo, wp, obbs, dets, rows_, extras)


def section(out, name, candidates, windows, calls):
    obb, plain, co, cp, _keep = entries(predictions(9, candidates))
    t = Timer()
    for f in (plain, obb):
        t.window(f, 2)
    runs = {"axis-aligned (yardstick)": [], "oriented": []}
    for _ in range(windows):
        runs["axis-aligned (yardstick)"].append(t.window(plain, calls))
        runs["oriented"].append(t.window(obb, calls))
    kept_o, kept_p = co.to_numpy((N,), np.int32).mean(), cp.to_numpy((N,), np.int32).mean()
    out.append("%s: %d x %d x %d, %d candidates / image (%.2e pair slots / call); kept %.0f (oriented) and %.0f (axis-aligned) / image; %d windows of %d calls, "
               "interleaved" % (name, N, ROWS, 4 + CLASSES + 1, candidates, N * candidates * (candidates - 1) / 2, kept_o, kept_p, windows, calls))
    for k, v in runs.items():
        out.append("    %-26s %s" % (k, stats(v)))
    p = np.asarray(runs["axis-aligned (yardstick)"])
    out.append("    spread of the yardstick's windows: %.2f %% (quartiles) of its median; oriented / axis-aligned medians: %.4f" % (
        100 * (np.percentile(p, 75) - np.percentile(p, 25)) / np.median(p), np.median(runs["oriented"]) / np.median(p)))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="", help="realistic | all")
    ap.add_argument("--out", default="", help="append the lines to this file as well")
    a = ap.parse_args()
    lines = []
    if a.only in ("", "realistic"):
        section(lines, "realistic", 300, 15, 20)
    if a.only in ("", "all"):
        section(lines, "all", ROWS, 7, 2)
    print("\n".join(lines))
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")
