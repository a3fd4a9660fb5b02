"""tools/bench_reduce.py -- speed of si_hip_reduce_* (include/si_reduce.h) against code that already exists and is not under test.

mean over H and W, channels kept, of [32,20,20,512], [32,7,7,512] and [8,160,160,64], fp32 and fp16:
    l  si_hip_reduce, the col_lane form forced
    c  si_hip_reduce, the col_coop form forced
    p  si_hip_adaptive_avgpool2d at output 1x1 on the same tensor (the kernel behind nn.AdaptiveAvgPool2d(1))
    b  si_hip_pad2d with zero pads on the same tensor: one read (and one write) of the same bytes
  The two forms can be forced in the EXPERIMENT build of the kernel library only (python -m simpleinfer_amd.build --experiment, then
  SI_HIP_LIB=build_variants/libsi_hip_exp.so), through SI_REDUCE_FORCE_COL = 1 / 2; with the product library the candidates are
    a  si_hip_reduce as the header's rule chooses
  and p, b.  The rule's own choice is printed for every shape either way.
mean and amax over C of [8,80,80,128] and [8,80,80,21], fp32 and fp16:
    a  si_hip_reduce (row_group)       b  the si_hip_pad2d copy
Each candidate set is timed in one process in alternating windows of >= --seconds, --repeats repeats; prints each window, the medians,
the spreads and the ratios to the last candidate and to p.  Bytes are counted from shapes (the input once; the copy moves them twice);
tensors below 256 MiB can live in the Infinity Cache, so bytes / time is not an HBM bandwidth there.
Run on an otherwise idle card, every GPU step under its own time limit:
  timeout -k 10 600 python tools/bench_reduce.py > profiles/reduce_<sha>.txt
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

POOL_SHAPES = [(32, 20, 20, 512), (32, 7, 7, 512), (8, 160, 160, 64)]
ROW_SHAPES = [(8, 80, 80, 128), (8, 80, 80, 21)]
HBM_BPS = 6.3e12
EXPERIMENT = "exp" in os.path.basename(_native.LIB_HIP_PATH)


class Case:
    """device operands and one launch of: "reduce" (force: None / 1 lane / 2 coop) | "pool" | "copy" """

    def __init__(self, kind, shape, half, op="mean", axes=6, force=None):
        self.H = H = _native.hip()
        self.kind, self.half, self.force = kind, half, force
        dt = np.float16 if half else np.float32
        x = np.random.default_rng(0).standard_normal(shape).astype(dt)
        self.dx = DeviceBuffer.from_numpy(x)
        self.bytes = x.nbytes
        n, h, w, c = shape
        tag = "%s %s" % ("fp16" if half else "fp32", "x".join(str(s) for s in shape))
        if kind == "reduce":
            self.d = hipops.reduce_desc(shape, op, axes)
            self.dy = DeviceBuffer(int(np.prod(hipops.reduce_out_shape(shape, axes))) * x.itemsize + 16)
            self._env()
            self.kernel = H.si_hip_reduce_kernel_name(C.byref(self.d), self.dx.ptr, self.dy.ptr, 1 if half else 0).decode()
            self.fn = H.si_hip_reduce_f16 if half else H.si_hip_reduce_f32
            self.name = "%s mask %d %s" % (op, axes, tag)
        elif kind == "pool":
            self.dy = DeviceBuffer(n * c * x.itemsize + 16)
            self.kernel = "adaptive_avgpool2d 1x1"
            self.fn = H.si_hip_adaptive_avgpool2d_f16 if half else H.si_hip_adaptive_avgpool2d_f32
            self.args = (self.dx.ptr, n, h, w, c, c, self.dy.ptr, 1, 1, c, None)
            self.name = "pool %s" % tag
        else:
            self.dy = DeviceBuffer(x.nbytes + 16)
            self.d = hipops.pad2d_desc(shape, (0, 0, 0, 0))
            self.kernel = H.si_hip_pad2d_kernel_name(C.byref(self.d), self.dx.ptr, self.dy.ptr, 1 if half else 0).decode()
            self.fn = H.si_hip_pad2d_f16 if half else H.si_hip_pad2d_f32
            self.name = "copy %s" % tag

    def _env(self):
        if self.force is None:
            os.environ.pop("SI_REDUCE_FORCE_COL", None)
        else:
            os.environ["SI_REDUCE_FORCE_COL"] = str(self.force)

    def begin(self):
        """before a window of launches of this case (the experiment library reads the switch at every launch)"""
        if self.kind == "reduce":
            self._env()

    def launch(self):
        if self.kind == "pool":
            _chk(self.fn(*self.args), self.name)
        else:
            _chk(self.fn(C.byref(self.d), self.dx.ptr, self.dy.ptr, None), self.name)


class Timer:
    def __init__(self):
        H = _native.hip()
        self.H = H
        self.e0, self.e1 = C.c_void_p(), C.c_void_p()
        _chk(H.si_hip_event_create(C.byref(self.e0)), "event")
        _chk(H.si_hip_event_create(C.byref(self.e1)), "event")

    def time(self, case, iters):
        H = self.H
        case.begin()
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


def compare(T, tags, cases, args):
    """alternating windows of the candidates; prints them and the ratios of each to the last one (the copy) and to p (the pool)"""
    for _ in range(2):   # warm-up
        for c in cases:
            T.window(c, 0.02)
    times = [[] for _ in cases]
    for _ in range(args.repeats):
        for c, t in zip(cases, times):
            t.append(T.window(c, args.seconds))
    med = [float(np.median(t)) for t in times]
    print(cases[0].name)
    for tag, c, t, m in zip(tags, cases, times, med):
        print("    %s [%-36s] %s ms   median %.4f ms  input bytes / time %.2f TB/s = %.0f %% of %.1f  spread %.1f %%" % (
            tag, c.kernel, " ".join("%.4f" % v for v in t), m, c.bytes / m * 1e-9, 100 * c.bytes / m * 1e3 / HBM_BPS, HBM_BPS * 1e-12,
            100 * (max(t) - min(t)) / m))
    line = "   ".join("%s / %s = %.3f" % (tag, tags[-1], m / med[-1]) for tag, m in zip(tags[:-1], med[:-1]))
    if "p" in tags:
        line += "   " + "   ".join("%s / p = %.3f" % (tag, m / med[tags.index("p")]) for tag, m in zip(tags, med) if tag not in "pb")
    print("    " + line, flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--seconds", type=float, default=0.2)
    args = ap.parse_args()
    T = Timer()
    print("HIP-event windows >= %.2f s, %d alternating repeats.  kernel library: %s (%s)" % (
        args.seconds, args.repeats, os.path.relpath(_native.LIB_HIP_PATH, ROOT), "experiment build: forms forced" if EXPERIMENT else "product build: the rule's form only"))
    for shape in POOL_SHAPES:
        for half in (False, True):
            rule = Case("reduce", shape, half)
            print("the rule's choice for %s %s: %s" % ("fp16" if half else "fp32", "x".join(map(str, shape)), rule.kernel))
            if EXPERIMENT:
                compare(T, "lcpb", [Case("reduce", shape, half, force=1), Case("reduce", shape, half, force=2), Case("pool", shape, half),
                                    Case("copy", shape, half)], args)
            else:
                compare(T, "apb", [rule, Case("pool", shape, half), Case("copy", shape, half)], args)
    os.environ.pop("SI_REDUCE_FORCE_COL", None)
    for shape in ROW_SHAPES:
        for half in (False, True):
            for op in ("mean", "amax"):
                compare(T, "ab", [Case("reduce", shape, half, op=op, axes=8), Case("copy", shape, half)], args)


if __name__ == "__main__":
    main()
