"""tools/bench_pixel_shuffle.py -- speed of si_hip_pixel_shuffle_f32 / _f16 against a copy of the same bytes, and of si_hip_prelu
against the LeakyReLU activation kernel.

Per shape three launches are compared in one process: (a) the form the launcher takes for 16-byte aligned dense buffers, (e) the
element form on the same tensors -- forced by handing the entry pointers one element off a 16-byte boundary, which is how the launcher
decides -- and (b) the yardstick: si_hip_pad2d with zero pads on the input tensor, a pure copy of the same byte count that already
exists and is not code under test.  For PReLU: (a) si_hip_prelu with per-channel slopes, (e) with one shared slope, (b)
si_hip_activation (LeakyReLU) on the same tensor.  Each is warmed up, then timed with HIP events over windows of >= --seconds,
a, e, b in turn, --repeats times.  Prints each window, the medians, the spreads and the ratios.  Bytes are counted from shapes (one
read + one write of the tensor); tensors below 256 MiB can live in the Infinity Cache, so bytes / time is not an HBM bandwidth there.
  shuffle:   [8,128,128,256] -> [8,256,256,64] (the SRResNet / EDSR upsampler), [8,256,256,48] -> C = 3, r = 4, [8,360,640,27] -> r = 3
  unshuffle: [8,512,512,3] -> 12 channels (Real-ESRGAN's x2 head)
  PReLU:     [8,256,256,64]
Run on an otherwise idle card, every GPU step under its own time limit:
  timeout -k 10 600 python tools/bench_pixel_shuffle.py > profiles/pixelshuffle_<sha>.txt
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

# (input NHWC shape, r, inverse)
SHAPES = [((8, 128, 128, 256), 2, False), ((8, 256, 256, 48), 4, False), ((8, 360, 640, 27), 3, False), ((8, 512, 512, 3), 2, True)]
PRELU_SHAPE = (8, 256, 256, 64)
HBM_BPS = 6.3e12


class Case:
    """device operands and one launch of: "shuffle" | "shuffle_elem" | "copy" | "prelu" | "prelu_shared" | "leakyrelu" """

    def __init__(self, kind, shape, r=1, inverse=False, half=False):
        self.H = H = _native.hip()
        self.kind, self.half = kind, half
        dt = np.float16 if half else np.float32
        es = 2 if half else 4
        x = np.random.default_rng(0).standard_normal(shape).astype(dt)
        self.c, self.pixels = shape[-1], int(np.prod(shape[:-1]))
        off = es if kind == "shuffle_elem" else 0          # one element off the 16-byte boundary: the launcher takes the element form
        self.dx, self.dy = DeviceBuffer(x.nbytes + 16), DeviceBuffer(x.nbytes + 16)
        _chk(H.si_hip_memcpy_h2d(self.dx.ptr + off, x.ctypes.data_as(C.c_void_p), x.nbytes, None), "h2d")
        _chk(H.si_hip_stream_sync(None), "sync")
        self.px, self.py = self.dx.ptr + off, self.dy.ptr + off
        self.bytes = 2 * x.nbytes
        tag = "x".join(str(s) for s in shape)
        if kind in ("shuffle", "shuffle_elem"):
            self.d = hipops.pixel_shuffle_desc(shape, r, inverse)
            self.kernel = H.si_hip_pixel_shuffle_kernel_name(C.byref(self.d), self.px, self.py, 1 if half else 0).decode()
            self.fn = H.si_hip_pixel_shuffle_f16 if half else H.si_hip_pixel_shuffle_f32
            self.name = "%s r=%d %s %s" % ("unshuffle" if inverse else "shuffle", r, "fp16" if half else "fp32", tag)
        elif kind == "copy":
            self.d = hipops.pad2d_desc(shape, (0, 0, 0, 0))
            self.kernel = H.si_hip_pad2d_kernel_name(C.byref(self.d), self.px, self.py, 1 if half else 0).decode()
            self.fn = H.si_hip_pad2d_f16 if half else H.si_hip_pad2d_f32
            self.name = "copy %s %s" % ("fp16" if half else "fp32", tag)
        elif kind in ("prelu", "prelu_shared"):
            count = self.c if kind == "prelu" else 1
            self.count = count
            self.ds = DeviceBuffer.from_numpy(np.linspace(0.05, 0.4, count).astype(np.float32))
            self.kernel = H.si_hip_prelu_kernel_name(self.px, self.pixels, self.c, self.c, count, self.py, self.c, 1 if half else 0).decode()
            self.name = "%s %s %s" % (kind, "fp16" if half else "fp32", tag)
        else:
            self.kernel = "activation (leakyrelu)"
            self.name = "leakyrelu %s %s" % ("fp16" if half else "fp32", tag)

    def launch(self):
        H = self.H
        if self.kind in ("shuffle", "shuffle_elem", "copy"):
            rc = self.fn(C.byref(self.d), self.px, self.py, None)
        elif self.kind in ("prelu", "prelu_shared"):
            rc = (H.si_hip_prelu_f16 if self.half else H.si_hip_prelu_f32)(self.px, self.pixels, self.c, self.c, self.ds.ptr, self.count, self.py, self.c, None)
        else:
            fn = H.si_hip_activation_f16 if self.half else H.si_hip_activation_f32
            rc = fn(hipops.ACT["leakyrelu"], 0.2, self.px, self.pixels, self.c, self.c, self.py, self.c, None)
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


def compare(T, trio, args):
    """alternating windows of a, e and b; prints them and returns the medians"""
    for _ in range(2):   # warm-up
        for c in trio:
            T.window(c, 0.05)
    times = [[] for _ in trio]
    for _ in range(args.repeats):
        for c, t in zip(trio, times):
            t.append(T.window(c, args.seconds)[0])
    med = [float(np.median(t)) for t in times]
    a = trio[0]
    print("%s" % a.name)
    for tag, c, t, m in zip("aeb", trio, times, med):
        print("    %s [%-34s] %s ms   median %.4f ms  bytes / time %.2f TB/s = %.0f %% of %.1f  spread %.1f %%" % (
            tag, c.kernel, " ".join("%.4f" % v for v in t), m, c.bytes / m * 1e-9, 100 * c.bytes / m * 1e3 / HBM_BPS, HBM_BPS * 1e-12,
            100 * (max(t) - min(t)) / m))
    print("    a / b = %.3f   e / b = %.3f   a / e = %.3f" % (med[0] / med[2], med[1] / med[2], med[0] / med[1]), flush=True)
    return med


def trios(prelu=True):
    """(a, e, b) of the default run, built one at a time"""
    for half in (False, True):
        for shape, r, inverse in SHAPES:
            yield Case("shuffle", shape, r, inverse, half), Case("shuffle_elem", shape, r, inverse, half), Case("copy", shape, half=half)
    for half in (False, True) if prelu else ():
        yield Case("prelu", PRELU_SHAPE, half=half), Case("prelu_shared", PRELU_SHAPE, half=half), Case("leakyrelu", PRELU_SHAPE, half=half)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--shuffle-only", action="store_true", help="skip the PReLU cases (a second run on a variant kernel library, SI_HIP_LIB)")
    args = ap.parse_args()
    if args.profile:
        for trio in trios():
            for _ in range(20):
                for c in trio:
                    c.launch()
            _chk(_native.hip().si_hip_device_sync(), "sync")
        print("profile: 20 launches of every candidate and yardstick")
        return
    T = Timer()
    print("HIP-event windows >= %.2f s, %d alternating repeats.  shuffle: a = the launcher's form, e = the element form (pointers one element off "
          "16 bytes), b = si_hip_pad2d with zero pads on the input tensor (a copy).  PReLU: a = per-channel slopes, e = one shared slope, "
          "b = si_hip_activation (LeakyReLU)" % (args.seconds, args.repeats))
    print("kernel library: %s" % _native.LIB_HIP_PATH)
    for trio in trios(not args.shuffle_only):
        compare(T, trio, args)


if __name__ == "__main__":
    main()
