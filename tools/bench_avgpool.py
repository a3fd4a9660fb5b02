"""tools/bench_avgpool.py -- speed of si_hip_avgpool2d_f32 / _f16 (include/si_pool.h), batch 8.

Default run: per shape the candidate (a) and its yardstick (b) are warmed up, then timed with HIP events over windows of >= --seconds,
a then b, --repeats times in one process (tools/bench_upsample.py's Timer / compare).  Prints each window, the medians, their ratio and
the spread of both.  Bytes are counted from shapes (input read once + output written); these tensors fit the 256 MiB Infinity Cache, so
"bytes / time" is not an HBM bandwidth.
  windowed form against si_hip_maxpool2d_f32 / _f16 with the same (k, s, p) on the same tensor -- the same bytes and the same tap count:
      56 x 56 x 128 k2 s2 (the DenseNet transition), 35 x 35 x 192 k3 s1 p1 without the pad in the divisor (the Inception branch),
      28 x 28 x 256 k2 s2, and 27 x 27 x 256 k2 s2 with ceil_mode and without the pad (ResNet-D; yardstick: the max pool of the 28 x 28 map,
      which has the same 14 x 14 output)
  cooperative form against si_hip_adaptive_avgpool2d_f32 / _f16 to (1, 1) over the same input bytes (global_avgpool_kernel):
      60 x 80 x 960 k49 s(16, 20) (LR-ASPP), adaptive 65 x 65 x 512 -> 6 x 6 and -> 2 x 2 (PSPNet)
  Expectation, not a test: a <= 1.25 b (DESIGN.md sections 9b / 9d / 9e).
--sweep: the form switch.  Square k x k windows, stride k // 2, on 64 x 64 x 256, k = 4 .. 32, through BOTH forms.  Only the experiment
build of the kernel library reads SI_AVGPOOL_COOP_TAPS (python -m simpleinfer_amd.build --experiment, selected with SI_HIP_LIB=...): the tool
sets it to 1 (every window cooperative) and to 2^30 (every window windowed) around the launches and refuses to run on the product
library, where the switch is the header's constant.  Prints per k both times and their ratio, and the smallest tap count from which the
cooperative form stays ahead.
--profile: launches every case a few times (for a rocprofv3 --kernel-trace --stats run of its own).
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

N = 8
BAR = 1.25
# (ih, iw, c, k, s, p, ceil_mode, count_include_pad, yardstick's (ih, iw))
WINDOWED = [(56, 56, 128, 2, 2, 0, False, True, None), (35, 35, 192, 3, 1, 1, False, False, None), (28, 28, 256, 2, 2, 0, False, True, None),
            (27, 27, 256, 2, 2, 0, True, False, (28, 28))]
# (ih, iw, c, k, s) or (ih, iw, c, adaptive output)
COOPERATIVE = [(60, 80, 960, (49, 49), (16, 20)), (65, 65, 512, (6, 6)), (65, 65, 512, (2, 2))]
SWEEP_SHAPE, SWEEP_K = (64, 64, 256), (4, 6, 8, 10, 12, 14, 16, 20, 24, 28, 32)


class Case:
    """device operands and one launch of: "avg" (the candidate) | "max" | "global" (the yardsticks)"""

    def __init__(self, kind, ih, iw, c, half=False, k=None, s=None, p=0, ceil_mode=False, count_include_pad=True, adaptive=None):
        self.H = _native.hip()
        self.kind, self.half = kind, half
        dt = np.float16 if half else np.float32
        x = np.random.default_rng(0).standard_normal((N, ih, iw, c)).astype(dt)
        self.dx = DeviceBuffer.from_numpy(x)
        self.shape = x.shape
        if kind == "global":
            oh = ow = 1
        elif adaptive is not None:
            self.d = hipops.adaptive_avgpool2d_desc(x.shape, adaptive)
            oh, ow = adaptive
        else:
            self.d = hipops.avgpool2d_desc(x.shape, k, s, p, ceil_mode, count_include_pad)
            oh, ow = self.d.oh, self.d.ow
            if kind == "max":
                kh, kw = hipops._pair(k)
                sh, sw = hipops._pair(s)
                ph, pw = hipops._pair(p)
                self.d = _native.SiPool2dDesc(N, ih, iw, c, c, oh, ow, c, kh, kw, sh, sw, 1, 1, ph, pw)
        out_bytes = N * oh * ow * c * x.itemsize
        self.dy = DeviceBuffer(out_bytes)
        self.bytes = x.nbytes + out_bytes
        what = "-> %dx%d" % tuple(adaptive) if adaptive is not None else ("-> 1x1" if kind == "global" else "k%s s%s p%s%s%s" % (
            k, s, p, " ceil" if ceil_mode else "", "" if count_include_pad else " nopad"))
        self.name = "%s %s %dx%dx%d %s" % (kind, "fp16" if half else "fp32", ih, iw, c, what)

    def kernel(self):
        return self.H.si_hip_avgpool2d_kernel_name(C.byref(self.d), self.dx.ptr, self.dy.ptr, 1 if self.half else 0).decode()

    def launch(self):
        H, (n, ih, iw, c) = self.H, self.shape
        if self.kind == "avg":
            rc = (H.si_hip_avgpool2d_f16 if self.half else H.si_hip_avgpool2d_f32)(C.byref(self.d), self.dx.ptr, self.dy.ptr, None)
        elif self.kind == "max":
            rc = (H.si_hip_maxpool2d_f16 if self.half else H.si_hip_maxpool2d_f32)(C.byref(self.d), self.dx.ptr, self.dy.ptr, None)
        else:
            rc = (H.si_hip_adaptive_avgpool2d_f16 if self.half else H.si_hip_adaptive_avgpool2d_f32)(self.dx.ptr, n, ih, iw, c, c, self.dy.ptr, 1, 1,
                                                                                                    c, None)
        _chk(rc, self.name)


def cases():
    """(candidate, yardstick, bar) triples of the default run, built one at a time"""
    for half in (False, True):
        for ih, iw, c, k, s, p, ce, cip, yard in WINDOWED:
            a = Case("avg", ih, iw, c, half, k, s, p, ce, cip)
            a.name += " [%s]" % a.kernel()
            yh, yw = yard or (ih, iw)
            yield a, Case("max", yh, yw, c, half, k, s, p), BAR
        for spec in COOPERATIVE:
            ih, iw, c = spec[:3]
            a = Case("avg", ih, iw, c, half, adaptive=spec[3]) if len(spec) == 4 else Case("avg", ih, iw, c, half, spec[3], spec[4])
            a.name += " [%s]" % a.kernel()
            yield a, Case("global", ih, iw, c, half), BAR


def sweep(T, args):
    lib = os.path.basename(_native.LIB_HIP_PATH)
    os.environ["SI_AVGPOOL_COOP_TAPS"] = "1"
    probe = Case("avg", 8, 8, 8, False, 2, 2, 0)
    if "coop" not in probe.kernel():
        sys.exit("--sweep needs the experiment build of the kernel library (SI_HIP_LIB=build_variants/libsi_hip_exp.so): %s ignores "
                 "SI_AVGPOOL_COOP_TAPS" % lib)
    ih, iw, c = SWEEP_SHAPE
    print("form sweep on %d x %d x %d x %d, k x k windows, stride k // 2; windows >= %.1f s, %d alternating repeats (a = cooperative, b = windowed)" %
          (N, ih, iw, c, args.seconds, args.repeats))

    class Forced:
        def __init__(self, case, taps):
            self.case, self.taps, self.bytes = case, taps, case.bytes
            os.environ["SI_AVGPOOL_COOP_TAPS"] = taps
            self.name = case.name + " [%s]" % case.kernel()

        def launch(self):
            os.environ["SI_AVGPOOL_COOP_TAPS"] = self.taps
            self.case.launch()

    rows = []
    for half in (False, True):
        for k in SWEEP_K:
            case = Case("avg", ih, iw, c, half, k, max(k // 2, 1), 0)
            r = compare(T, Forced(case, "1"), Forced(case, str(1 << 30)), args, None)
            rows.append((half, k * k, r))
    for half in (False, True):
        mine = [(t, r) for h, t, r in rows if h == half]
        ahead = [t for i, (t, r) in enumerate(mine) if all(r2 < 1.0 for _, r2 in mine[i:])]
        print("%s: cooperative / windowed by taps: %s; cooperative stays ahead from %s taps" % (
            "fp16" if half else "fp32", "  ".join("%d: %.2f" % tr for tr in mine), ahead[0] if ahead else "(never in this range)"))
    del os.environ["SI_AVGPOOL_COOP_TAPS"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--sweep", action="store_true")
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
    if args.sweep:
        sweep(T, args)
        return
    print("batch %d, HIP-event windows >= %.1f s, %d alternating repeats (a = candidate, b = the max pool of the same window / the global mean "
          "of the same input)" % (N, args.seconds, args.repeats))
    worst, missed = 0.0, []
    for a, b, bar in cases():
        r = compare(T, a, b, args, bar)
        worst = max(worst, r)
        if r > bar:
            missed.append(a.name)
    print("worst a/b = %.3f (expectation %.2f); above it: %s" % (worst, BAR, ", ".join(missed) if missed else "none"))


if __name__ == "__main__":
    main()
