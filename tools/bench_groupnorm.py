"""tools/bench_groupnorm.py -- speed of si_hip_groupnorm_f32 / _f16 (batch 8) against si_hip_batchnorm2d_f32 on the same tensor.

Per shape the candidate (a) and the yardstick (b) -- si_hip_batchnorm2d_f32 on an fp32 tensor of the same shape: one read plus one
write, the traffic a normalisation cannot go below -- are warmed up, then timed with HIP events over windows of >= --seconds, a then
b, --repeats times in one process.  Prints each window, the medians, the spreads and the ratio.  The fp16 candidates are held to the
yardstick's time scaled by the byte ratio (0.5).  Bytes are counted from shapes (one read + one write of the tensor); most of these
tensors fit the 256 MiB Infinity Cache, so bytes / time is not an HBM bandwidth.
  GroupNorm, 32 groups: 128^2 x 128, 64^2 x 256, 32^2 x 512, 16^2 x 1024;  InstanceNorm: 128^2 x 64, 64^2 x 128;  fp32 and fp16
  expectation: two-launch form (two reads + one write) a <= 1.5 * 1.25 b; one-launch form a <= 1.25 b
Run on an otherwise idle card, every GPU step under its own time limit, the steps chained:
  timeout -k 10 600 python tools/bench_groupnorm.py > profiles/groupnorm_<sha>.txt && timeout -k 10 120 python tools/bench_groupnorm.py --profile
With the experiment build of the kernel library (python -m simpleinfer_amd.build --experiment; SI_HIP_LIB=build_variants/libsi_hip_exp.so)
SI_GROUPNORM_FORM=2 runs the two-launch form on the shapes that take one launch: the A/B behind the form rule.
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
GROUP = [(128, 128, 128, 32), (64, 64, 256, 32), (32, 32, 512, 32), (16, 16, 1024, 32)]   # h, w, c, groups
INSTANCE = [(128, 128, 64, 64), (64, 64, 128, 128)]
HBM_BPS = 6.3e12
MARGIN = 1.25


class Case:
    """device operands and one launch of: "groupnorm" | "batchnorm" (the yardstick, fp32 only)"""

    def __init__(self, kind, h, w, c, groups, half=False):
        self.H = _native.hip()
        self.kind, self.half = kind, half
        dt = np.float16 if half else np.float32
        x = np.random.default_rng(0).standard_normal((N, h, w, c)).astype(dt)
        self.c, self.pixels = c, N * h * w
        self.dx, self.dy = DeviceBuffer.from_numpy(x), DeviceBuffer(x.nbytes)
        self.bytes = 2 * x.nbytes
        rng = np.random.default_rng(1)
        self.par = [DeviceBuffer.from_numpy(rng.uniform(0.5, 1.5, c).astype(np.float32)) for _ in range(4)]   # mean, var, gamma, beta
        self.d = hipops.group_norm_desc(x.shape, groups, affine=True)
        self.ws = None
        if kind == "groupnorm":
            nbytes = self.H.si_hip_groupnorm_workspace_bytes(C.byref(self.d))
            self.ws = DeviceBuffer(nbytes) if nbytes else None
            self.kernel = self.H.si_hip_groupnorm_kernel_name(C.byref(self.d), self.dx.ptr, self.dy.ptr, 1 if half else 0).decode()
            self.launches = 1 if self.ws is None else 2
        else:
            self.kernel, self.launches = "batchnorm2d", 1
        self.name = "%s %s %dx%dx%d g%d" % (kind, "fp16" if half else "fp32", h, w, c, groups)

    def launch(self):
        H = self.H
        if self.kind == "groupnorm":
            fn = H.si_hip_groupnorm_f16 if self.half else H.si_hip_groupnorm_f32
            rc = fn(C.byref(self.d), self.dx.ptr, self.par[2].ptr, self.par[3].ptr, self.dy.ptr, self.ws.ptr if self.ws else None, None)
        else:
            rc = H.si_hip_batchnorm2d_f32(self.dx.ptr, self.pixels, self.c, self.c, self.par[0].ptr, self.par[1].ptr, self.par[2].ptr, self.par[3].ptr,
                                          1e-5, self.dy.ptr, self.c, None)
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
    """alternating windows of a and b; prints them and returns (ratio to the byte-scaled yardstick, bar)"""
    for _ in range(2):   # warm-up
        T.window(a, 0.1)
        T.window(b, 0.1)
    ta, tb = [], []
    for _ in range(args.repeats):
        ta.append(T.window(a, args.seconds)[0])
        tb.append(T.window(b, args.seconds)[0])
    ma, mb = float(np.median(ta)), float(np.median(tb))
    scale = a.bytes / b.bytes                         # 0.5 for the fp16 candidates
    bar = MARGIN * (1.5 if a.launches == 2 else 1.0)
    ratio = ma / (mb * scale)
    print("%-34s [%s]" % (a.name, a.kernel))
    print("    a: %s ms   b: %s ms" % (" ".join("%.4f" % t for t in ta), " ".join("%.4f" % t for t in tb)))
    print("    median a %.4f ms (bytes / time %.2f TB/s = %.0f %% of %.1f; spread %.1f %%)  b %.4f ms (%.2f TB/s, spread %.1f %%)  "
          "a / (b x %.1f) = %.3f  (expectation <= %.3f)%s" %
          (ma, a.bytes / ma * 1e-9, 100 * a.bytes / ma * 1e3 / HBM_BPS, HBM_BPS * 1e-12, 100 * (max(ta) - min(ta)) / ma, mb, b.bytes / mb * 1e-9,
           100 * (max(tb) - min(tb)) / mb, scale, ratio, bar, "  ok" if ratio <= bar else "  ABOVE"))
    return ratio, bar


def cases():
    """(candidate, yardstick) pairs of the default run, built one at a time"""
    for half in (False, True):
        for (h, w, c, g) in GROUP + INSTANCE:
            yield Case("groupnorm", h, w, c, g, half), Case("batchnorm", h, w, c, g)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--profile", action="store_true")
    args = ap.parse_args()
    if args.profile:
        for a, b in cases():
            for _ in range(20):
                a.launch()
                b.launch()
            _chk(_native.hip().si_hip_device_sync(), "sync")
        print("profile: 20 launches of every candidate and yardstick")
        return
    T = Timer()
    print("batch %d, HIP-event windows >= %.1f s, %d alternating repeats (a = si_hip_groupnorm, b = si_hip_batchnorm2d_f32 on the fp32 tensor "
          "of the same shape)" % (N, args.seconds, args.repeats))
    missed = []
    for a, b in cases():
        r, bar = compare(T, a, b, args)
        if r > bar:
            missed.append("%s (%.2f)" % (a.name, r))
    print("above the expectation: %s" % (", ".join(missed) if missed else "none"))


if __name__ == "__main__":
    main()
