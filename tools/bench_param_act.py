"""tools/bench_param_act.py -- speed of si_hip_param_act_* (include/si_act.h) against code that already exists and is not under test.

[32,112,112,32] and [32,7,7,1280] (MobileNetV2's first and last activations) and [8,80,80,128], fp32 and fp16, dense:
    c  si_hip_param_act clamp(0, 6)          m  si_hip_param_act mish          s  si_hip_param_act softplus(1, 20)
    r  si_hip_activation relu on the same tensor: the same bytes, the kernel this one is modelled on
    u  si_hip_activation silu on the same tensor
    b  si_hip_pad2d with zero pads on the same tensor: one read and one write of the same bytes
Each candidate set is timed in one process in alternating windows of >= --seconds, --repeats repeats; prints each window, the medians,
the spreads and the ratios c / r, m / u, s / u and each to the copy.  Bytes are counted from shapes (read once, written once); tensors
below 256 MiB can live in the Infinity Cache, so bytes / time is not an HBM bandwidth there.
Run on an otherwise idle card, every GPU step under its own time limit:
  timeout -k 10 600 python tools/bench_param_act.py > profiles/param_act_<sha>.txt
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

SHAPES = [(32, 112, 112, 32), (32, 7, 7, 1280), (8, 80, 80, 128)]
HBM_BPS = 6.3e12


class Case:
    """device operands and one launch of: "param" (op, p0, p1) | "act" (kind) | "copy" """

    def __init__(self, kind, shape, half, op=None, p0=0.0, p1=0.0):
        self.H = H = _native.hip()
        self.kind = kind
        dt = np.float16 if half else np.float32
        x = (np.random.default_rng(0).standard_normal(shape) * 3.0).astype(dt)
        self.dx = DeviceBuffer.from_numpy(x)
        self.dy = DeviceBuffer(x.nbytes + 16)
        self.bytes = 2 * x.nbytes
        c = shape[-1]
        pixels = x.size // c
        tag = "%s %s" % ("fp16" if half else "fp32", "x".join(str(s) for s in shape))
        if kind == "param":
            self.d = hipops.param_act_desc(shape, op, p0, p1)
            self.kernel = H.si_hip_param_act_kernel_name(C.byref(self.d), self.dx.ptr, self.dy.ptr, 1 if half else 0).decode()
            self.fn = H.si_hip_param_act_f16 if half else H.si_hip_param_act_f32
            self.args = (C.byref(self.d), self.dx.ptr, self.dy.ptr, None)
            self.name = "%s %s" % (op, tag)
        elif kind == "act":
            self.kernel = "activation %s" % op
            self.fn = H.si_hip_activation_f16 if half else H.si_hip_activation_f32
            self.args = (hipops.ACT[op], 0.0, self.dx.ptr, pixels, c, c, self.dy.ptr, c, None)
            self.name = "%s %s" % (op, tag)
        else:
            self.d = hipops.pad2d_desc(shape, (0, 0, 0, 0))
            self.kernel = H.si_hip_pad2d_kernel_name(C.byref(self.d), self.dx.ptr, self.dy.ptr, 1 if half else 0).decode()
            self.fn = H.si_hip_pad2d_f16 if half else H.si_hip_pad2d_f32
            self.args = (C.byref(self.d), self.dx.ptr, self.dy.ptr, None)
            self.name = "copy %s" % tag
        self.tag = tag

    def launch(self):
        _chk(self.fn(*self.args), self.name)


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
        return ms / iters


PAIRS = (("c", "r"), ("m", "u"), ("s", "u"))   # the candidate and the yardstick it should sit with


def compare(T, tags, cases, args):
    """alternating windows of the candidates; prints them, the ratios of each new op to its yardstick and of everything to the copy"""
    for _ in range(2):   # warm-up
        for c in cases:
            T.window(c, 0.02)
    times = [[] for _ in cases]
    for _ in range(args.repeats):
        for c, t in zip(cases, times):
            t.append(T.window(c, args.seconds))
    med = dict(zip(tags, (float(np.median(t)) for t in times)))
    print(cases[0].tag)
    for tag, c, t in zip(tags, cases, times):
        m = med[tag]
        print("    %s [%-38s] %s ms   median %.4f ms  bytes / time %.2f TB/s = %.0f %% of %.1f  spread %.1f %%" % (
            tag, c.kernel, " ".join("%.4f" % v for v in t), m, c.bytes / m * 1e-9, 100 * c.bytes / m * 1e3 / HBM_BPS, HBM_BPS * 1e-12,
            100 * (max(t) - min(t)) / m))
    print("    " + "   ".join("%s / %s = %.3f" % (a, b, med[a] / med[b]) for a, b in PAIRS) + "   |   " +
          "   ".join("%s / b = %.3f" % (t, med[t] / med["b"]) for t in tags if t != "b"), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--seconds", type=float, default=0.2)
    args = ap.parse_args()
    T = Timer()
    print("HIP-event windows >= %.2f s, %d alternating repeats.  kernel library: %s" % (args.seconds, args.repeats, os.path.relpath(_native.LIB_HIP_PATH, ROOT)))
    for shape in SHAPES:
        for half in (False, True):
            compare(T, "cmsrub", [Case("param", shape, half, "clamp", 0.0, 6.0), Case("param", shape, half, "mish"),
                                  Case("param", shape, half, "softplus", 1.0, 20.0), Case("act", shape, half, "relu"), Case("act", shape, half, "silu"),
                                  Case("copy", shape, half)], args)


if __name__ == "__main__":
    main()
