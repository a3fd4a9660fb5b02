"""tools/bench_upsample.py -- speed of si_hip_upsample_bilinear_f32 / _f16 and si_hip_segment_labels_* (batch 8).

Default run: per shape the candidate (a) and its yardstick (b) -- si_hip_upsample_nearest_f32 on the same input, size and strides, which
moves exactly the bytes the bilinear kernel must move; for fp16 the nearest kernel called with c / 2 words, as the Upsample layer calls
it -- are warmed up, then timed with HIP events over windows of >= 1 s, a then b, --repeats times in one process.  Prints each window, the
medians, their ratio and the spread.  Bytes are counted from shapes (n ih iw c + n oh ow c elements; label map: n ih iw c elements +
n oh ow bytes); "bytes / time" is printed next to the 6.3 TB/s achievable HBM bandwidth, but most of these tensors fit the 256 MiB
Infinity Cache, so it is not an HBM bandwidth.
  decoder shapes (c % 4 == 0, x2, both align_corners):  bar a <= 1.25 b, fp32 and fp16
  head shapes (c = 21, 64^2 -> 512^2 and 65^2 -> 513^2): no bar for the copy kernel; the label map must take less time than b
--profile: launches every case a few times (for a rocprofv3 --kernel-trace --stats run of its own).
"""
import argparse
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from simpleinfer_amd import _native, hipops  # noqa: E402
from simpleinfer_amd.hipops import DeviceBuffer, _chk  # noqa: E402

N = 8
DECODER = [(16, 16, 1024), (32, 32, 512), (64, 64, 256), (128, 128, 128)]   # ih, iw, c; output 2x
HEADS = [((64, 64, 21), (512, 512), False), ((65, 65, 21), (513, 513), True)]
HBM_BPS = 6.3e12
BAR = 1.25


class Case:
    """device operands and one launch of: "bilinear" | "nearest" (the yardstick) | "labels" """

    def __init__(self, kind, ih, iw, c, out_hw, ac, half=False):
        self.H = _native.hip()
        self.kind, self.half, self.c = kind, half, c
        dt = np.float16 if half else np.float32
        x = np.random.default_rng(0).standard_normal((N, ih, iw, c)).astype(dt)
        self.ih, self.iw = ih, iw
        self.d = hipops.upsample_desc(x.shape, out_hw=out_hw, align_corners=ac)
        self.dx = DeviceBuffer.from_numpy(x)
        out_px = N * out_hw[0] * out_hw[1]
        if kind == "labels":
            self.dy = DeviceBuffer(out_px)
            self.bytes = x.nbytes + out_px
        else:
            self.dy = DeviceBuffer(out_px * c * x.itemsize)
            self.bytes = x.nbytes + out_px * c * x.itemsize
        # the yardstick's scale factors: it forms its own steps as 1 / scale; its index rule needs no align_corners
        self.scale = (np.float32(out_hw[0]) / np.float32(ih), np.float32(out_hw[1]) / np.float32(iw))
        self.name = "%s %s %dx%dx%d -> %dx%d%s" % (kind, "fp16" if half else "fp32", ih, iw, c, out_hw[0], out_hw[1], " ac" if ac else "")

    def launch(self):
        H, d = self.H, self.d
        if self.kind == "bilinear":
            fn = H.si_hip_upsample_bilinear_f16 if self.half else H.si_hip_upsample_bilinear_f32
            rc = fn(C.byref(d), self.dx.ptr, self.dy.ptr, None)
        elif self.kind == "labels":
            fn = H.si_hip_segment_labels_f16 if self.half else H.si_hip_segment_labels_f32
            rc = fn(C.byref(d), self.dx.ptr, self.dy.ptr, None)
        else:
            words = self.c // 2 if self.half else self.c   # (fp16: pure data movement as 4-byte words, as layer/upsample.cpp does)
            rc = H.si_hip_upsample_nearest_f32(self.dx.ptr, d.n, d.ih, d.iw, words, words, self.scale[0], self.scale[1], self.dy.ptr, d.oh, d.ow,
                                               words, None)
        _chk(rc, self.name)


class Timer:
    def __init__(self):
        H = _native.hip()
        self.H = H
        self.e0, self.e1 = C.c_void_p(), C.c_void_p()
        _chk(H.si_hip_event_create(C.byref(self.e0)), "event")
        _chk(H.si_hip_event_create(C.byref(self.e1)), "event")

    def time(self, case, iters):
        H = self.H
        _chk(H.si_hip_event_record(self.e0, None), "record")
        for _ in range(iters):
            case.launch()
        _chk(H.si_hip_event_record(self.e1, None), "record")
        _chk(H.si_hip_event_sync(self.e1), "sync")
        ms = C.c_float()
        _chk(H.si_hip_event_elapsed_ms(self.e0, self.e1, C.byref(ms)), "elapsed")
        return ms.value

    def window(self, case, seconds):
        """mean ms per launch over one window of >= `seconds`"""
        est = self.time(case, 10) / 10
        iters = max(20, int(seconds * 1000.0 / max(est, 1e-3)) + 1)
        ms = self.time(case, iters)
        while ms < seconds * 1000.0:   # (the estimate ran short: lengthen the window)
            iters = int(iters * seconds * 1000.0 / max(ms, 1e-3) * 1.1) + 1
            ms = self.time(case, iters)
        return ms / iters, iters


def compare(T, a, b, args, bar):
    """alternating windows of a and b; prints them and returns median(a) / median(b)"""
    for _ in range(2):   # warm-up
        T.window(a, 0.1)
        T.window(b, 0.1)
    ta, tb = [], []
    for _ in range(args.repeats):
        ta.append(T.window(a, args.seconds)[0])
        tb.append(T.window(b, args.seconds)[0])
    ma, mb = float(np.median(ta)), float(np.median(tb))
    verdict = "" if bar is None else ("  ok" if ma / mb <= bar else "  ABOVE %.2f" % bar)
    print("%-46s a: %s ms  b: %s ms" % (a.name, " ".join("%.4f" % t for t in ta), " ".join("%.4f" % t for t in tb)))
    print("    median a %.4f ms (bytes / time %.2f TB/s = %.0f %% of %.1f; spread %.1f %%)  b %.4f ms (%.2f TB/s, spread %.1f %%)  a/b = %.3f%s" %
          (ma, a.bytes / ma * 1e-9, 100 * a.bytes / ma * 1e3 / HBM_BPS, HBM_BPS * 1e-12, 100 * (max(ta) - min(ta)) / ma, mb, b.bytes / mb * 1e-9,
           100 * (max(tb) - min(tb)) / mb, ma / mb, verdict))
    return ma / mb


def cases():
    """(candidate, yardstick, bar) triples of the default run, built one at a time"""
    for half in (False, True):
        for (ih, iw, c) in DECODER:
            for ac in (False, True):
                hw = (2 * ih, 2 * iw)
                yield Case("bilinear", ih, iw, c, hw, ac, half), Case("nearest", ih, iw, c, hw, False, half), BAR
    for (ih, iw, c), hw, ac in HEADS:
        yield Case("bilinear", ih, iw, c, hw, ac), Case("nearest", ih, iw, c, hw, False), None
        yield Case("labels", ih, iw, c, hw, ac), Case("nearest", ih, iw, c, hw, False), 1.0
        yield Case("labels", ih, iw, c, hw, ac, True), Case("nearest", ih, iw, c, hw, False), 1.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--profile", action="store_true")
    args = ap.parse_args()
    if args.profile:
        for a, b, _ in cases():
            for _ in range(20):
                a.launch()
                b.launch()
            _chk(_native.hip().si_hip_device_sync(), "sync")
        print("profile: 20 launches of every candidate and yardstick")
        return
    T = Timer()
    print("batch %d, HIP-event windows >= %.1f s, %d alternating repeats (a = candidate, b = si_hip_upsample_nearest_f32 on the same bytes)" %
          (N, args.seconds, args.repeats))
    worst, missed = 0.0, []
    for a, b, bar in cases():
        r = compare(T, a, b, args, bar)
        if bar == BAR:
            worst = max(worst, r)
        if bar is not None and r > bar:
            missed.append(a.name)
    print("decoder shapes: worst a/b = %.3f (bar %.2f); missed bars: %s" % (worst, BAR, ", ".join(missed) if missed else "none"))


if __name__ == "__main__":
    main()
