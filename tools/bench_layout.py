"""tools/bench_layout.py -- speed of the three forms of si_hip_permute_* (include/si_permute.h) at head-sized shapes against two yardsticks
that exist without it and are not code under test.

Shapes: feature maps of 80x80, 40x40 and 20x20 with 255 and 144 channels, batch 1 and 32, fp32 and fp16.  Per shape, each candidate set timed
in one process in alternating windows:
  t  permute_tile   the NHWC -> [N, C, H W] transpose of view(N, C, -1): nest [N, C, HW], strides [HW C, 1, C]
  e  permute_elem   the same nest through the element form
  r  permute_rows   the raw YOLOv5 head's view -> permute -> view: nest [N, 3, HW, C / 3], runs of C / 3
  c  si_hip_copy_channels_f32 moving the same bytes (fp16: as 4-byte words): the yardstick every ratio is taken against
  n  si_hip_nhwc_to_nchw_f32, the element loop behind torch.flatten, on the same transpose (fp32 only: it has no fp16 form)
Windows of >= --seconds, --repeats alternating repeats; prints each window's mean, the medians, bytes / time (one read + one write, counted
from shapes) and the ratios to c.  Tensors below 256 MiB can live in the Infinity Cache, so bytes / time is not an HBM bandwidth there.
Run on an otherwise idle card under a time limit:
  timeout -k 10 600 python tools/bench_layout.py > profiles/layout_<sha>.txt
--switch times the tile form against the element form with one tile dimension at 2 .. 64 (the other at 6400, batch 8): where SI_PERMUTE_TILE_MIN
belongs.  --lds-probe runs ONE permute_tile launch per type and nothing else: the process to put under a counter run (SQ_LDS_BANK_CONFLICT) of its own.
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

HBM_BPS = 6.3e12


class Case:
    def __init__(self, kind, n, hw, c, half, swap=False):
        self.H = H = _native.hip()
        self.kind, self.half = kind, half
        es = 2 if half else 4
        count = n * hw * c
        self.bytes = 2 * count * es
        self.dx, self.dy = DeviceBuffer(count * es), DeviceBuffer(count * es)
        self.dx.fill(0x3C)
        self.name = "%s [%d, %d, %d] %s" % (kind, n, hw, c, "fp16" if half else "fp32")
        if kind in ("tile", "elem") and swap:     # the short dimension is the input-contiguous one
            self.d = hipops.permute_desc((n, hw, c), (hw * c, 1, hw), form=kind)
        elif kind in ("tile", "elem"):
            self.d = hipops.permute_desc((n, c, hw), (hw * c, 1, c), form=kind)
        elif kind == "rows":
            self.d = hipops.permute_desc((n, 3, hw, c // 3), (hw * c, c // 3, c, 1), form="rows")
        if kind in ("tile", "elem", "rows"):
            self.fn = H.si_hip_permute_f16 if half else H.si_hip_permute_f32
            self.kernel = H.si_hip_permute_kernel_name(C.byref(self.d), self.dx.ptr, self.dy.ptr, 1 if half else 0).decode()
        elif kind == "copy":
            self.words, self.kernel = count * es // 4, "copy_channels_kernel"
            self.width = 64                      # the dense copy as rows of up to 64 words: the largest power of two that divides it
            while self.words % self.width:
                self.width //= 2
        else:
            self.dims, self.kernel = (n, hw, 1, c), "nhwc_to_nchw_kernel"

    def launch(self):
        H = self.H
        if self.kind in ("tile", "elem", "rows"):
            _chk(self.fn(C.byref(self.d), self.dx.ptr, self.dy.ptr, None), self.name)
        elif self.kind == "copy":
            _chk(H.si_hip_copy_channels_f32(self.dx.ptr, self.words // self.width, self.width, self.width, self.dy.ptr, self.width, None), self.name)
        else:
            n, h, w, c = self.dims
            _chk(H.si_hip_nhwc_to_nchw_f32(self.dx.ptr, n, h, w, c, c, self.dy.ptr, None), self.name)


class Timer:
    def __init__(self):
        self.H = H = _native.hip()
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
        while ms < seconds * 1000.0:
            iters = int(iters * seconds * 1000.0 / max(ms, 1e-3) * 1.1) + 1
            ms = self.time(case, iters)
        return ms / iters


def compare(T, tags, cases, args):
    for c in cases:   # warm-up
        T.window(c, 0.02)
    times = [[] for _ in cases]
    for _ in range(args.repeats):
        for c, t in zip(cases, times):
            t.append(T.window(c, args.seconds))
    med = [float(np.median(t)) for t in times]
    yard = med[tags.index("c")]
    for tag, c, t, m in zip(tags, cases, times, med):
        print("    %s %-34s [%-26s] median %.4f ms  %.2f TB/s = %2.0f %% of %.1f  spread %4.1f %%  / c = %.2f" % (
            tag, c.name, c.kernel, m, c.bytes / m * 1e-9, 100 * c.bytes / m * 1e3 / HBM_BPS, HBM_BPS * 1e-12, 100 * (max(t) - min(t)) / m, m / yard))
    sys.stdout.flush()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--seconds", type=float, default=0.1)
    ap.add_argument("--maps", type=int, nargs="*", default=[80, 40, 20])
    ap.add_argument("--channels", type=int, nargs="*", default=[255, 144])
    ap.add_argument("--batches", type=int, nargs="*", default=[1, 32])
    ap.add_argument("--lds-probe", action="store_true")
    ap.add_argument("--switch", action="store_true")
    args = ap.parse_args()
    if args.lds_probe:
        for half in (False, True):
            Case("tile", 32, 6400, 256, half).launch()
        _chk(_native.hip().si_hip_device_sync(), "sync")
        print("lds probe: two permute_tile launches, [32, 256, 6400] fp32 and fp16")
        return
    T = Timer()
    if args.switch:
        print("tile / elem with one tile dimension short (the other 6400, batch 8); short = the output-contiguous one, then the input-contiguous one")
        for half in (False, True):
            for swap in (False, True):
                for ext in (2, 3, 4, 6, 8, 12, 16, 32, 64):
                    cases = [Case(k, 8, 6400, ext, half, swap) for k in ("tile", "elem")]
                    for c in cases:
                        T.window(c, 0.02)
                    t = [float(np.median([T.window(c, args.seconds) for _ in range(args.repeats)])) for c in cases]
                    print("    %s short %s = %2d   tile %.4f ms   elem %.4f ms   tile / elem = %.2f" % (
                        "fp16" if half else "fp32", "in " if swap else "out", ext, t[0], t[1], t[0] / t[1]), flush=True)
        return
    print("HIP-event windows >= %.2f s, %d alternating repeats.  kernel library: %s" % (args.seconds, args.repeats, _native.LIB_HIP_PATH))
    for half in (False, True):
        for s in args.maps:
            for c in args.channels:
                for n in args.batches:
                    kinds = ["tile", "elem", "rows", "copy"] + ([] if half else ["nchw"])
                    tags = "terc" + ("" if half else "n")
                    compare(T, tags, [Case(k, n, s * s, c, half) for k in kinds], args)


if __name__ == "__main__":
    main()
