"""tools/bench_conv_transpose.py -- speed of si_hip_conv_transpose2d_f32 on U-Net decoder up-convs (batch 8 from a 256x256 image).

Default run: for each k2 s2 up-conv shape, the new kernel (a) and its yardstick (b) -- si_hip_conv2d_f32 as a 1x1 conv Cin -> 4*Cout on the same
input: the same FLOPs, the same input read, the same bytes written -- are warmed up, then timed with HIP events over windows of >= 1 s, a then b,
--repeats times in one process.  Prints each window, the medians, their ratio and the spread; then the k3 s2 p1 op1 and k4 s2 p1 forms at the
same shapes (event-timed, no bar) with achieved TF/s against the fp32 MFMA peak (157.3 TF/s) and HBM (8 TB/s) bounds.
--profile-forms: only launches the k3 / k4 forms a few times each (for a rocprofv3 --kernel-trace --stats run of its own).
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
SHAPES = [(16, 16, 1024, 512), (32, 32, 512, 256), (64, 64, 256, 128), (128, 128, 128, 64)]   # H, W, Cin, Cout
FORMS = {"k2s2": ((2, 2), (2, 2), (0, 0), (0, 0)), "k3s2p1op1": ((3, 3), (2, 2), (1, 1), (1, 1)), "k4s2p1": ((4, 4), (2, 2), (1, 1), (0, 0))}
PEAK_FLOPS, HBM_BPS = 157.3e12, 8e12


class Case:
    """device operands and one launch of the transposed conv (form) or of the 1x1 yardstick"""

    def __init__(self, h, w, cin, cout, form=None, yardstick=False):
        H = _native.hip()
        self.H = H
        rng = np.random.default_rng(0)
        x = rng.uniform(-1, 1, (N, h, w, cin)).astype(np.float32)
        self.dx = DeviceBuffer.from_numpy(x)
        if yardstick:
            oc = 4 * cout
            a = np.sqrt(3.0 / cin)
            wt = rng.uniform(-a, a, (oc, cin, 1, 1)).astype(np.float32)
            self.d = hipops.SiConv2dDesc(N, h, w, cin, cin, h, w, oc, oc, 1, 1, 1, 1, 1, 1, 0, 0, 1, 1, 0, 0, oc, 0, 0.0)
            packed = np.zeros(H.si_hip_conv2d_weight_elems(C.byref(self.d)), np.float32)
            _chk(H.si_hip_conv2d_pack_weight_host(C.byref(self.d), wt.ctypes.data_as(C.c_void_p), packed.ctypes.data_as(C.c_void_p)), "pack")
            self.out_elems = N * h * w * oc
            self.flops = 2.0 * N * h * w * cin * oc
            self.name = "1x1 conv %d->%d" % (cin, oc)
        else:
            k, s, p, op = FORMS[form]
            a = np.sqrt(3.0 / (cin * k[0] * k[1]))
            wt = rng.uniform(-a, a, (cin, cout, k[0], k[1])).astype(np.float32)
            self.d = hipops.conv_transpose2d_desc(x.shape, wt.shape, True, s, p, op)
            packed = hipops.conv_transpose2d_pack(self.d, wt)
            self.out_elems = N * self.d.oh * self.d.ow * cout
            self.flops = 2.0 * N * h * w * cin * cout * k[0] * k[1]
            self.name = "%s %d->%d" % (form, cin, cout)
        self.yardstick = yardstick
        self.dw = DeviceBuffer.from_numpy(packed)
        self.db = DeviceBuffer.from_numpy(rng.uniform(-0.1, 0.1, (4 * cout,)).astype(np.float32))   # (4 Cout: enough for either)
        self.dy = DeviceBuffer(self.out_elems * 4)
        self.bytes = (x.nbytes + self.out_elems * 4 + packed.nbytes)

    def launch(self):
        if self.yardstick:
            rc = self.H.si_hip_conv2d_f32(C.byref(self.d), self.dx.ptr, self.dw.ptr, self.db.ptr, None, self.dy.ptr, None)
        else:
            rc = self.H.si_hip_conv_transpose2d_f32(C.byref(self.d), self.dx.ptr, self.dw.ptr, self.db.ptr, self.dy.ptr, None)
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
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--profile-forms", action="store_true")
    args = ap.parse_args()
    if args.profile_forms:
        for form in ("k3s2p1op1", "k4s2p1"):
            for (h, w, cin, cout) in SHAPES:
                c = Case(h, w, cin, cout, form)
                for _ in range(20):
                    c.launch()
        _chk(_native.hip().si_hip_device_sync(), "sync")
        print("profile-forms: 20 launches of each k3s2p1op1 / k4s2p1 shape")
        return
    T = Timer()
    print("batch %d, HIP-event windows >= %.1f s, %d alternating repeats (a = conv_transpose k2 s2, b = 1x1 conv Cin -> 4 Cout)" %
          (N, args.seconds, args.repeats))
    worst = 0.0
    for (h, w, cin, cout) in SHAPES:
        a, b = Case(h, w, cin, cout, "k2s2"), Case(h, w, cin, cout, yardstick=True)
        for _ in range(3):   # warm-up
            T.window(a, 0.2)
            T.window(b, 0.2)
        ta, tb = [], []
        for r in range(args.repeats):
            ta.append(T.window(a, args.seconds)[0])
            tb.append(T.window(b, args.seconds)[0])
        ma, mb = float(np.median(ta)), float(np.median(tb))
        worst = max(worst, ma / mb)
        print("%3dx%-3d %4d->%-4d  a: %s ms  b: %s ms" % (h, w, cin, cout, " ".join("%.4f" % t for t in ta), " ".join("%.4f" % t for t in tb)))
        print("          median a %.4f ms (%.1f TF/s, spread %.1f %%)  b %.4f ms (%.1f TF/s, spread %.1f %%)  a/b = %.3f  %s" %
              (ma, a.flops / ma * 1e-9, 100 * (max(ta) - min(ta)) / ma, mb, b.flops / mb * 1e-9, 100 * (max(tb) - min(tb)) / mb, ma / mb,
               "ok" if ma / mb <= 1.25 else "ABOVE 1.25"))
    print("worst a/b = %.3f (bar 1.25)" % worst)
    print("\nother forms (no bar; event-timed, %.1f s windows, median of %d)" % (args.seconds, args.repeats))
    for form in ("k3s2p1op1", "k4s2p1"):
        for (h, w, cin, cout) in SHAPES:
            c = Case(h, w, cin, cout, form)
            T.window(c, 0.2)
            t = float(np.median([T.window(c, args.seconds)[0] for _ in range(args.repeats)]))
            tf = c.flops / t * 1e-9
            t_mfma, t_hbm = c.flops / PEAK_FLOPS * 1e3, c.bytes / HBM_BPS * 1e3
            lim = "MFMA" if t_mfma >= t_hbm else "HBM"
            print("%-10s %3dx%-3d %4d->%-4d  %.4f ms  %.1f TF/s  bound %s %.4f ms: %.0f %% of it" %
                  (form, h, w, cin, cout, t, tf, lim, max(t_mfma, t_hbm), 100 * max(t_mfma, t_hbm) / t))


if __name__ == "__main__":
    main()
