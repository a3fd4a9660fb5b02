"""tools/bench_deform_conv.py -- speed of si_hip_deform_conv2d_f32 at detector-neck sizes (batch 32, 3x3 pad 1, with a mask, one offset group).

For each shape the deformable conv (a) and its ceiling (b) -- si_hip_conv2d_f32, the implicit-GEMM family (not Winograd), at the same shape: the
same MFMA work without the gather -- are warmed up, then timed with HIP events over windows of >= --seconds, a then b, --repeats times in one
process.  Prints each window, the medians with their spread, TFLOP/s, the ratio a / b, and the ratio of a to its byte floor (x once, offsets +
mask once, the output once, at 8 TB/s).  A third kernel (c) is timed beside them: si_hip_conv_transpose2d_f32 as 3x3 stride 1 pad 1 at the same
shape -- the tile skeleton the deformable conv shares (64 x 64, one LDS stage) with plain 16-byte A loads where the gather is: what the
skeleton reaches without the gather.  --zero-offsets repeats the run with all offsets 0 (every sample is one pixel read four times over: the
gather's arithmetic without its scattered addresses), the evidence for what bounds the kernel.
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

N = 32
SHAPES = [(80, 80, 128, 128), (40, 40, 256, 256), (20, 20, 512, 512)]   # H, W, Cin, Cout
HBM_BPS = 8e12


class Case:
    """device operands and one launch of the deformable conv or of the plain conv at the same shape"""

    def __init__(self, h, w, cin, cout, plain=False, zero_offsets=False, skeleton=False):
        H = _native.hip()
        self.H = H
        rng = np.random.default_rng(0)
        x = rng.uniform(-1, 1, (N, h, w, cin)).astype(np.float32)
        a = np.sqrt(3.0 / (cin * 9))
        wt = rng.uniform(-a, a, (cout, cin, 3, 3)).astype(np.float32)
        self.dx = DeviceBuffer.from_numpy(x)
        self.plain, self.skeleton = plain, skeleton
        self.flops = 2.0 * N * h * w * cout * cin * 9
        if skeleton:
            wt = np.ascontiguousarray(wt.transpose(1, 0, 2, 3))
            self.d = hipops.conv_transpose2d_desc(x.shape, wt.shape, True, (1, 1), (1, 1))
            packed = hipops.conv_transpose2d_pack(self.d, wt)
            self.name = "conv_transpose 3x3 s1 p1 %d->%d" % (cin, cout)
        elif plain:
            self.d = _native.SiConv2dDesc(N, h, w, cin, cin, h, w, cout, cout, 3, 3, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, cout, 0, 0.0)
            packed = np.zeros(H.si_hip_conv2d_weight_elems(C.byref(self.d)), np.float32)
            _chk(H.si_hip_conv2d_pack_weight_host(C.byref(self.d), wt.ctypes.data_as(C.c_void_p), packed.ctypes.data_as(C.c_void_p)), "pack")
            self.name = "conv2d 3x3 %d->%d: %s" % (cin, cout, H.si_hip_conv2d_kernel_name(C.byref(self.d), C.c_void_p(self.dx.ptr)).decode())
            self.floor_bytes = x.nbytes + N * h * w * cout * 4
        else:
            off = (np.zeros((N, h, w, 18)) if zero_offsets else rng.uniform(-2.5, 2.5, (N, h, w, 18))).astype(np.float32)
            m = rng.uniform(0, 1, (N, h, w, 9)).astype(np.float32)
            self.d = hipops.deform_conv2d_desc(x.shape, off.shape, wt.shape, True, True, (1, 1), (1, 1))
            packed = hipops.deform_conv2d_pack(self.d, wt)
            self.do, self.dm = DeviceBuffer.from_numpy(off), DeviceBuffer.from_numpy(m)
            self.name = "deform conv 3x3 %d->%d%s" % (cin, cout, ", zero offsets" if zero_offsets else "")
            self.floor_bytes = x.nbytes + off.nbytes + m.nbytes + N * h * w * cout * 4
        self.dw = DeviceBuffer.from_numpy(packed)
        self.db = DeviceBuffer.from_numpy(rng.uniform(-0.1, 0.1, (cout,)).astype(np.float32))
        self.dy = DeviceBuffer(N * h * w * cout * 4)

    def launch(self):
        if self.skeleton:
            rc = self.H.si_hip_conv_transpose2d_f32(C.byref(self.d), self.dx.ptr, self.dw.ptr, self.db.ptr, self.dy.ptr, None)
        elif self.plain:
            rc = self.H.si_hip_conv2d_f32(C.byref(self.d), self.dx.ptr, self.dw.ptr, self.db.ptr, None, self.dy.ptr, None)
        else:
            rc = self.H.si_hip_deform_conv2d_f32(C.byref(self.d), self.dx.ptr, self.do.ptr, self.dm.ptr, self.dw.ptr, self.db.ptr, self.dy.ptr, None)
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--seconds", type=float, default=0.5)
    ap.add_argument("--zero-offsets", action="store_true")
    args = ap.parse_args()
    T = Timer()
    print("batch %d, 3x3 pad 1 with mask, HIP-event windows >= %.1f s, %d alternating repeats (a = deform conv, b = conv2d on the implicit GEMM)" %
          (N, args.seconds, args.repeats))
    for (h, w, cin, cout) in SHAPES:
        a, b, c = Case(h, w, cin, cout, zero_offsets=args.zero_offsets), Case(h, w, cin, cout, plain=True), Case(h, w, cin, cout, skeleton=True)
        for _ in range(2):   # warm-up
            T.window(a, 0.1)
            T.window(b, 0.1)
            T.window(c, 0.1)
        ta, tb, tc = [], [], []
        for r in range(args.repeats):
            ta.append(T.window(a, args.seconds)[0])
            tb.append(T.window(b, args.seconds)[0])
            tc.append(T.window(c, args.seconds)[0])
        ma, mb, mc = float(np.median(ta)), float(np.median(tb)), float(np.median(tc))
        floor = a.floor_bytes / HBM_BPS * 1e3
        print("%3dx%-3d %4d->%-4d  a (%s): %s ms  b (%s): %s ms" % (h, w, cin, cout, a.name, " ".join("%.4f" % t for t in ta), b.name,
                                                               " ".join("%.4f" % t for t in tb)))
        print("          median a %.4f ms (%.1f TF/s, spread %.1f %%)  b %.4f ms (%.1f TF/s, spread %.1f %%)  a/b = %.3f  a / byte floor (%.4f ms) = %.1f" %
              (ma, a.flops / ma * 1e-9, 100 * (max(ta) - min(ta)) / ma, mb, b.flops / mb * 1e-9, 100 * (max(tb) - min(tb)) / mb, ma / mb, floor,
               ma / floor))
        print("          c (%s): %s ms  median %.4f ms (%.1f TF/s)  a/c = %.3f" % (c.name, " ".join("%.4f" % t for t in tc), mc, c.flops / mc * 1e-9, ma / mc))


if __name__ == "__main__":
    main()
