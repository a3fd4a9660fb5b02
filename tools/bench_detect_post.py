"""tools/bench_detect_post.py -- measurements of the general detection post-processing (include/si_detect.h).  Run on the GPU.

  (a) si_hip_detect_postprocess_f32 in YOLOv5 mode against si_hip_yolo_postprocess_f32 on the same 32 x 25200 x 85 predictions with a few hundred
      survivors per image: windows of back-to-back calls between two device events, the two entries alternating window by window in one process;
      the median window of each, and the spread of the old entry's windows.
  (b) the filter at 32 x 8400 x 84 and 32 x 8400 x 116 in both layouts: the call time of the whole entry here; the filter KERNEL's time comes from
      `rocprofv3 --kernel-trace --stats -- python tools/bench_detect_post.py --only b:<k>` (one configuration per process, so that the
      statistics of a kernel name belong to one shape).  The bytes the filter has to read are computed here from the shapes.
  (c) si_hip_detect_masks_f32 on 32 images of 160 x 160 x 32 prototypes with 10 / 100 / 300 detections per image and boxes of 5 - 40 % of the
      image: time per call, mask bytes written per second, and the share of (pixel, detection) pairs whose wave formed the dot.

Every number is a time on the device ended by an event; nothing here asserts."""
import argparse
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from simpleinfer_amd import _native, hipops  # noqa: E402
from util import synthetic_predictions  # noqa: E402

HBM_MEASURED = 6.29e12      # bytes / s, a float4 copy on this chip (the microarchitecture notes); the spec sheet says 8.0e12


class Timer:
    def __init__(self):
        self.H = _native.hip()
        self.e0, self.e1 = C.c_void_p(), C.c_void_p()
        hipops._chk(self.H.si_hip_event_create(C.byref(self.e0)), "event")
        hipops._chk(self.H.si_hip_event_create(C.byref(self.e1)), "event")

    def window(self, call, calls):
        """ms per call over `calls` back-to-back calls on the null stream"""
        ms = C.c_float()
        self.H.si_hip_event_record(self.e0, None)
        for _ in range(calls):
            call()
        self.H.si_hip_event_record(self.e1, None)
        self.H.si_hip_event_sync(self.e1)
        self.H.si_hip_event_elapsed_ms(self.e0, self.e1, C.byref(ms))
        return ms.value / calls


def stats(v):
    v = np.sort(np.asarray(v))
    return "median %.4f ms (min %.4f, quartiles %.4f .. %.4f, max %.4f)" % (np.median(v), v[0], v[len(v) // 4], v[(3 * len(v)) // 4], v[-1])


class Post:
    """one configuration of the general entry with its buffers"""

    def __init__(self, pred_storage, n, rows, classes, objectness, extra, layout, thr, max_det=300):
        self.H = _native.hip()
        self.d = hipops.detect_desc(n, rows, classes, objectness, extra, layout, "cxcywh", thr, 0.45, False, max_det)
        self.pred = hipops.DeviceBuffer.from_numpy(pred_storage)
        self.ws = hipops.DeviceBuffer(hipops.detect_workspace_bytes(self.d))
        self.bufs = [hipops.DeviceBuffer(max(n * max_det * k * 4, 16)) for k in (6, 1, 4, max(extra, 1))]
        self.cnt = hipops.DeviceBuffer(n * 4)
        dets, rows_, boxes, extras = self.bufs
        self.out = _native.SiDetectPostOut(dets.ptr, self.cnt.ptr, rows_.ptr, boxes.ptr, extras.ptr)
        self.n = n

    def __call__(self):
        rc = self.H.si_hip_detect_postprocess_f32(C.byref(self.d), self.pred.ptr, None, C.byref(self.out), self.ws.ptr, self.ws.nbytes, None)
        assert rc == 0, rc

    def counts(self):
        return self.cnt.to_numpy((self.n,), np.int32)


def section_a(out, windows=21, calls=20):
    H = _native.hip()
    n, rows, ne = 32, 25200, 85
    pred = synthetic_predictions(3, n, rows, nc=80, n_gt=8, hot_frac=0.015)
    survivors = float(((pred[..., 4] * pred[..., 5:].max(-1)) >= 0.25).sum()) / n
    new = Post(pred, n, rows, 80, True, 0, "rows", 0.25)
    wsb = H.si_hip_yolo_postprocess_workspace_bytes(n, rows, ne)
    ws, dets, cnt = hipops.DeviceBuffer(wsb), hipops.DeviceBuffer(n * 300 * 24), hipops.DeviceBuffer(n * 4)

    def old():
        rc = H.si_hip_yolo_postprocess_f32(new.pred.ptr, n, rows, ne, 0.25, 0.45, 0, None, dets.ptr, cnt.ptr, 300, ws.ptr, wsb, None)
        assert rc == 0, rc

    # the general entry with nothing optional asked for: the old entry's work exactly
    bare = Post(pred, n, rows, 80, True, 0, "rows", 0.25)
    bare.out = _native.SiDetectPostOut(bare.bufs[0].ptr, bare.cnt.ptr, None, None, None)
    t = Timer()
    for f in (old, new, bare):
        t.window(f, 5)
    same = dets.to_numpy((n, 300, 6)).tobytes() == new.bufs[0].to_numpy((n, 300, 6)).tobytes() and cnt.to_numpy((n,), np.int32).tobytes() == new.counts().tobytes()
    runs = {"old": [], "new": [], "new, no optional outputs": []}
    for _ in range(windows):
        for name, f in (("old", old), ("new", new), ("new, no optional outputs", bare)):
            runs[name].append(t.window(f, calls))
    out.append("(a) %d x %d x %d, %.0f survivors / image, %.1f boxes / image; same bytes: %s; %d windows of %d calls each, interleaved" % (
        n, rows, ne, survivors, new.counts().mean(), same, windows, calls))
    for name, v in runs.items():
        out.append("    %-26s %s" % (name, stats(v)))
    o = np.asarray(runs["old"])
    out.append("    spread of the old entry's windows: %.2f %% (quartiles) / %.2f %% (min .. max) of its median; new / old medians: %.4f, bare / old: %.4f" % (
        100 * (np.percentile(o, 75) - np.percentile(o, 25)) / np.median(o), 100 * (o.max() - o.min()) / np.median(o),
        np.median(runs["new"]) / np.median(o), np.median(runs["new, no optional outputs"]) / np.median(o)))


FILTER_CONFIGS = [(80, 0, "rows"), (80, 0, "channels"), (80, 32, "rows"), (80, 32, "channels")]


def filter_config(k):
    """32 x 8400 x (84 | 116), a few hundred survivors per image"""
    classes, extra, layout = FILTER_CONFIGS[k]
    n, rows = 32, 8400
    p5 = synthetic_predictions(5, n, rows, nc=classes, n_gt=8, hot_frac=0.04)
    pred = np.concatenate([p5[..., :4], p5[..., 4:5] * p5[..., 5:]], 2)               # no box score: the class scores carry the confidence
    if extra:
        pred = np.concatenate([pred, np.random.Generator(np.random.Philox(6)).random((n, rows, extra), dtype=np.float32)], 2)
    ne = 4 + classes + extra
    store = np.ascontiguousarray(pred if layout == "rows" else pred.transpose(0, 2, 1))
    # what the filter kernel has to read: ROWS stages the scanned part of every row (box + scores); CHANNELS reads the scores of every row
    # and the box of the survivors alone
    scan = n * rows * (4 + classes) * 4 if layout == "rows" else n * rows * classes * 4
    return Post(store, n, rows, classes, False, extra, layout, 0.25), ne, layout, scan, n * rows * ne * 4


def section_b(out, only=None, windows=15, calls=20):
    t = Timer()
    for k in range(len(FILTER_CONFIGS)) if only is None else [only]:
        post, ne, layout, scan, whole = filter_config(k)
        t.window(post, 5)
        v = [t.window(post, calls) for _ in range(windows)]
        out.append("(b) 32 x 8400 x %d %-8s %s: entry %s; %.0f boxes / image; the filter reads %.1f MB of the tensor's %.1f MB: %.1f us at %.2f TB/s" % (
            ne, layout, hipops.detect_filter_kernel_name(post.d, post.pred.ptr), stats(v), post.counts().mean(), scan / 1e6, whole / 1e6,
            scan / HBM_MEASURED * 1e6, HBM_MEASURED / 1e12))


MASK_COUNTS = (10, 100, 300)


def mask_config(k, n=32, mh=160, mw=160, nm=32, size=640):
    count = MASK_COUNTS[k]
    r = np.random.Generator(np.random.Philox(40 + k))
    protos = r.uniform(-1, 1, (n, mh, mw, nm)).astype(np.float32)
    extras = r.uniform(-1, 1, (n, count, nm)).astype(np.float32)
    wh = r.uniform(0.05, 0.4, (n, count, 2)) * size
    xy = r.uniform(0, 1, (n, count, 2)) * (size - wh)
    boxes = np.concatenate([xy, wh], 2).astype(np.float32)
    return protos, extras, boxes, np.full(n, count, np.int32), np.float32(mw) / np.float32(size)


def dot_share(boxes, ratio, mh, mw, images=4):
    """share of (pixel, detection) pairs in a wave that forms the dot: a wave is 64 consecutive pixels of the plane"""
    need = total = 0
    c, r = np.arange(mw, dtype=np.float32)[None, :], np.arange(mh, dtype=np.float32)[:, None]
    for b in range(images):
        for bx, by, bw, bh in boxes[b]:
            crop = (c >= bx * ratio) & (c < (bx + bw) * ratio) & (r >= by * ratio) & (r < (by + bh) * ratio)
            need += int(crop.reshape(-1, 64).any(1).sum()) * 64
            total += mh * mw
    return need / total


def section_c(out, only=None, windows=15, calls=10):
    H = _native.hip()
    t = Timer()
    for k in range(len(MASK_COUNTS)) if only is None else [only]:
        protos, extras, boxes, counts, ratio = mask_config(k)
        n, mh, mw, nm = protos.shape
        count = extras.shape[1]
        d = hipops.detect_mask_desc(n, mh, mw, nm, count, nm, 0, ratio, ratio)
        bufs = [hipops.DeviceBuffer.from_numpy(a) for a in (protos, extras, boxes, counts)]
        masks = hipops.DeviceBuffer(n * count * mh * mw)

        def call():
            rc = H.si_hip_detect_masks_f32(C.byref(d), bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, bufs[3].ptr, masks.ptr, None)
            assert rc == 0, rc

        t.window(call, 3)
        v = [t.window(call, calls) for _ in range(windows)]
        written = n * count * mh * mw
        share = dot_share(boxes, ratio, mh, mw)
        med = float(np.median(v))
        out.append("(c) 32 x 160 x 160 x 32, %3d detections / image, %s: %s; %.1f MB of masks: %.2f TB/s written (+ %.1f MB of prototypes read per call); "
                   "%.1f %% of the (pixel, detection) pairs formed a dot" % (count, hipops.detect_masks_kernel_name(d, bufs[0].ptr), stats(v), written / 1e6,
                                                                           written / (med * 1e-3) / 1e12, protos.nbytes / 1e6, 100 * share))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="", help="a | b | c | b:<k> | c:<k>: one section, or one configuration of it (for a profiler run)")
    ap.add_argument("--out", default="", help="append the lines to this file as well")
    a = ap.parse_args()
    lines = []
    sec, _, k = a.only.partition(":")
    k = int(k) if k else None
    if sec in ("", "a"):
        section_a(lines)
    if sec in ("", "b"):
        section_b(lines, k)
    if sec in ("", "c"):
        section_c(lines, k)
    print("\n".join(lines))
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")
