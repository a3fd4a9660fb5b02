"""tools/bench_softmax.py -- speed of si_hip_softmax_f32 / _f16 against the nn.Sigmoid activation kernel on the same tensor.

Per shape the candidate (a) and the yardstick (b) -- si_hip_activation_f32 / _f16 (sigmoid) on the same tensor in the same dtype: one
read plus one write and one exponential per element, the traffic of a single-read softmax; it is not code under test -- are warmed up,
then timed with HIP events over windows of >= --seconds, a then b, --repeats times in one process.  Prints each window, the medians,
the spreads and the ratio.  Bytes are counted from shapes (one read + one write of the tensor); most of these tensors fit the 256 MiB
Infinity Cache, so bytes / time is not an HBM bandwidth.
  the issue's shapes: [64,1,1,1000], [8,160,160,21], [8,160,160,256] on axis 3; [8,160,160,32] on axes 1 and 2
  the forms those do not reach: [2048,1,1,2048] (block), [1024,1,1,8192] (block_online), [8,8,3200,32] on axis 1 (strided, in registers)
  expectation: register-resident forms (group, block, strided) a ~ 1.0 b; re-reading forms (block_online, strided_online) a ~ 1.5 b
  (two reads + one write against one read + one write); a case is flagged ABOVE beyond 1.25 x that
Run on an otherwise idle card, every GPU step under its own time limit:
  timeout -k 10 600 python tools/bench_softmax.py > profiles/softmax_<sha>.txt
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

SHAPES = [((64, 1, 1, 1000), 3), ((8, 160, 160, 21), 3), ((8, 160, 160, 256), 3), ((8, 160, 160, 32), 1), ((8, 160, 160, 32), 2),
          ((2048, 1, 1, 2048), 3), ((1024, 1, 1, 8192), 3), ((8, 8, 3200, 32), 1)]
HBM_BPS = 6.3e12
MARGIN = 1.25


class Case:
    """device operands and one launch of: "softmax" | "sigmoid" (the yardstick)"""

    def __init__(self, kind, shape, axis, half=False, log=False):
        self.H = _native.hip()
        self.kind, self.half = kind, half
        dt = np.float16 if half else np.float32
        x = np.random.default_rng(0).standard_normal(shape).astype(dt)
        self.c, self.pixels = shape[3], shape[0] * shape[1] * shape[2]
        self.dx, self.dy = DeviceBuffer.from_numpy(x), DeviceBuffer(x.nbytes)
        self.bytes = 2 * x.nbytes
        self.d = hipops.softmax_desc(shape, axis, log)
        if kind == "softmax":
            self.kernel = self.H.si_hip_softmax_kernel_name(C.byref(self.d), self.dx.ptr, self.dy.ptr, 1 if half else 0).decode()
        else:
            self.kernel = "activation (sigmoid)"
        self.rereads = "online" in self.kernel
        self.name = "%s %s %s axis %d" % ("log_softmax" if log else kind, "fp16" if half else "fp32", "x".join(str(s) for s in shape), axis)

    def launch(self):
        H = self.H
        if self.kind == "softmax":
            rc = (H.si_hip_softmax_f16 if self.half else H.si_hip_softmax_f32)(C.byref(self.d), self.dx.ptr, self.dy.ptr, None)
        else:
            fn = H.si_hip_activation_f16 if self.half else H.si_hip_activation_f32
            rc = fn(hipops.ACT["sigmoid"], 0.0, self.dx.ptr, self.pixels, self.c, self.c, self.dy.ptr, self.c, None)
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


def compare(T, a, b, args):
    """alternating windows of a and b; prints them and returns (ratio to the yardstick, expectation)"""
    for _ in range(2):   # warm-up
        T.window(a, 0.05)
        T.window(b, 0.05)
    ta, tb = [], []
    for _ in range(args.repeats):
        ta.append(T.window(a, args.seconds)[0])
        tb.append(T.window(b, args.seconds)[0])
    ma, mb = float(np.median(ta)), float(np.median(tb))
    expect = 1.5 if a.rereads else 1.0
    ratio = ma / mb
    print("%-48s [%s]" % (a.name, a.kernel))
    print("    a: %s ms   b: %s ms" % (" ".join("%.4f" % t for t in ta), " ".join("%.4f" % t for t in tb)))
    print("    median a %.4f ms (bytes / time %.2f TB/s = %.0f %% of %.1f; spread %.1f %%)  b %.4f ms (%.2f TB/s, spread %.1f %%)  "
          "a / b = %.3f  (expectation ~ %.1f)%s" %
          (ma, a.bytes / ma * 1e-9, 100 * a.bytes / ma * 1e3 / HBM_BPS, HBM_BPS * 1e-12, 100 * (max(ta) - min(ta)) / ma, mb, b.bytes / mb * 1e-9,
           100 * (max(tb) - min(tb)) / mb, ratio, expect, "  ok" if ratio <= MARGIN * expect else "  ABOVE"), flush=True)
    return ratio, MARGIN * expect


def cases(with_log):
    """(candidate, yardstick) pairs of the default run, built one at a time"""
    for half in (False, True):
        for shape, axis in SHAPES:
            yield Case("softmax", shape, axis, half), Case("sigmoid", shape, axis, half)
    if with_log:
        for half in (False, True):
            yield Case("softmax", (8, 160, 160, 21), 3, half, log=True), Case("sigmoid", (8, 160, 160, 21), 3, half)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--profile", action="store_true")
    args = ap.parse_args()
    if args.profile:
        for a, b in cases(True):
            for _ in range(20):
                a.launch()
                b.launch()
            _chk(_native.hip().si_hip_device_sync(), "sync")
        print("profile: 20 launches of every candidate and yardstick")
        return
    T = Timer()
    print("HIP-event windows >= %.2f s, %d alternating repeats (a = si_hip_softmax, b = si_hip_activation sigmoid on the same tensor, same dtype)"
          % (args.seconds, args.repeats))
    missed = []
    for a, b in cases(True):
        r, bar = compare(T, a, b, args)
        if r > bar:
            missed.append("%s (%.2f)" % (a.name, r))
    print("above 1.25 x the expectation: %s" % (", ".join(missed) if missed else "none"))


if __name__ == "__main__":
    main()
