"""tools/bench_binary_const.py -- speed of si_hip_binary_const_f32 / _f16 (include/si_binary.h) on [32, 80, 80, 128] against a per-channel
constant [1, 1, 1, 128] (form chan), a per-position constant [1, 80, 80, 1] (form pixel) and a full-size per-image constant [1, 80, 80, 128]
(form full), one stage (x * c) and two (x * c0 + c1), fp32 and fp16.

Per case the candidate (a) and a yardstick (b) are warmed up, then timed with HIP events over alternating windows, --repeats times in one
process; the medians, their ratio and the spread are printed.  Yardsticks:
  copy     a device-to-device copy of x's size: one read and one write of the tensor, which the kernel must at least move
  parent   si_hip_binary_f32, the kernel these operands took before (fp32 only; two stages are two launches through an intermediate tensor)
Bytes are counted from shapes (x read + out written + each constant read once).  The fp16 tensor (52 MB) and its result fit the 256 MiB
Infinity Cache together, the fp32 pair (2 x 105 MB) nearly: "bytes / time" is printed next to the 6.3 TB/s achievable HBM bandwidth but is
not an HBM bandwidth.  Expectation, not a test: a <= b for the parent, and a within the constant's traffic of the copy.
"""
import argparse
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_upsample import Timer, compare  # noqa: E402
from simpleinfer_amd import _native, hipops  # noqa: E402
from simpleinfer_amd.hipops import DeviceBuffer, _chk  # noqa: E402

X = (32, 80, 80, 128)
CONSTS = {"chan": (1, 1, 1, 128), "pixel": (1, 80, 80, 1), "full": (1, 80, 80, 128)}


class Case:
    """device operands and one launch of: "const" (the candidate) | "copy" | "parent" """

    def __init__(self, kind, form, stages, half=False):
        self.H = _native.hip()
        self.kind, self.half, self.stages = kind, half, stages
        dt = np.float16 if half else np.float32
        rng = np.random.default_rng(0)
        x = rng.standard_normal(X).astype(dt)
        cs = CONSTS[form]
        self.consts = [DeviceBuffer.from_numpy((rng.random(cs) + 0.5).astype(dt)) for _ in range(stages)]
        self.dx = DeviceBuffer.from_numpy(x)
        self.dy = DeviceBuffer(x.nbytes)
        self.nbytes = x.nbytes
        self.bytes = 2 * x.nbytes + (0 if kind == "copy" else stages * int(np.prod(cs)) * x.itemsize)
        self.d = hipops.binary_const_desc(X, [2, 0][:stages], [cs] * stages)
        self.cs = (C.c_int * 4)(*cs)
        self.xs = (C.c_int * 4)(*X)
        self.name = "%s %s %s x%d" % (kind, "fp16" if half else "fp32", form, stages)
        if kind == "parent":
            self.mid = DeviceBuffer(x.nbytes) if stages == 2 else None
            self.bytes += (stages - 1) * 2 * x.nbytes
        if kind == "const":
            c1 = self.consts[1].ptr if stages == 2 else None
            self.name += " [%s]" % self.H.si_hip_binary_const_kernel_name(C.byref(self.d), self.dx.ptr, self.consts[0].ptr, c1, self.dy.ptr,
                                                                          1 if half else 0).decode()

    def launch(self):
        H = self.H
        if self.kind == "const":
            fn = H.si_hip_binary_const_f16 if self.half else H.si_hip_binary_const_f32
            rc = fn(C.byref(self.d), self.dx.ptr, self.consts[0].ptr, self.consts[1].ptr if self.stages == 2 else None, self.dy.ptr, None)
        elif self.kind == "copy":
            rc = H.si_hip_memcpy_d2d(self.dy.ptr, self.dx.ptr, self.nbytes, None)
        else:
            first = self.mid.ptr if self.stages == 2 else self.dy.ptr
            rc = H.si_hip_binary_f32(2, self.dx.ptr, self.xs, X[3], self.consts[0].ptr, self.cs, self.cs[3], first, self.xs, X[3], None)
            if rc == 0 and self.stages == 2:
                rc = H.si_hip_binary_f32(0, self.mid.ptr, self.xs, X[3], self.consts[1].ptr, self.cs, self.cs[3], self.dy.ptr, self.xs, X[3], None)
        _chk(rc, self.name)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--seconds", type=float, default=0.5)
    args = ap.parse_args()
    T = Timer()
    print("x %s, HIP-event windows >= %.1f s, %d alternating repeats (a = si_hip_binary_const, b = the yardstick named in its line)" % (
        X, args.seconds, args.repeats))
    slower = []
    for half in (False, True):
        for form in ("chan", "pixel", "full"):
            for stages in (1, 2):
                r = compare(T, Case("const", form, stages, half), Case("copy", form, stages, half), args, None)
                if not half:
                    p = compare(T, Case("const", form, stages, half), Case("parent", form, stages, half), args, 1.0)
                    if p > 1.0:
                        slower.append("fp32 %s x%d (%.3f)" % (form, stages, p))
                print("    -> %s %s x%d: %.3f of the copy's time" % ("fp16" if half else "fp32", form, stages, r))
    print("slower than the parent kernel: %s" % (", ".join(slower) if slower else "none"))


if __name__ == "__main__":
    main()
