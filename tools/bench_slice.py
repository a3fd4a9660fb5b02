"""tools/bench_slice.py -- speed of si_hip_split_channels_* and si_hip_slice_* (include/si_slice.h) against copies of the same bytes that
already exist and are not code under test, and of the aliased (alias_split=1) against the copied (alias_split=0) plan of a C2f block.

Kernels, fp32 and fp16, each candidate set timed in one process in alternating windows:
  split  [8,160,160,64] -> 2 x 32 channels
           a  si_hip_split_channels, the vec form (one launch)
           e  the same through the elem form (pointers one element off a 16-byte boundary, which is how the launcher decides)
           k  the K-call baseline: one si_hip_copy_channels_f32 per piece (fp16: as 4-byte words), which reads the input K times
           b  si_hip_pad2d with zero pads on the input tensor: one copy of the same bytes
  focus  [8,640,640,3] -> four step-2 slices [8,320,320,3]
           a  four si_hip_slice launches (the elem form: C = 3)
           b  si_hip_pad2d with zero pads on the input tensor: one copy of the same bytes
Engine: build_toy_c2f(batch, size, c1, c2, n) with alias_split 1 and 0, the two engines alive side by side and timed in turn
(Engine.last_forward_ms: HIP events around the launches of one forward, hipGraph replay), fp32 and fp16 storage.
Windows of >= --seconds, --repeats alternating repeats; prints each window, the medians, the spreads and the ratios.  Bytes are counted
from shapes (one read + one write); tensors below 256 MiB can live in the Infinity Cache, so bytes / time is not an HBM bandwidth there.
Run on an otherwise idle card, every GPU step under its own time limit:
  timeout -k 10 600 python tools/bench_slice.py > profiles/slice_<sha>.txt
"""
import argparse
import ctypes as C
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from simpleinfer_amd import _native, hipops, modelgen as mg  # noqa: E402
from simpleinfer_amd.engine import Engine  # noqa: E402
from simpleinfer_amd.hipops import DeviceBuffer, _chk  # noqa: E402

SPLIT_SHAPE, SPLIT_WIDTHS = (8, 160, 160, 64), (32, 32)
FOCUS_SHAPE = (8, 640, 640, 3)
HBM_BPS = 6.3e12
ALL = slice(None)


class Case:
    """device operands and one launch (or the launches of one candidate) of: "split" | "split_elem" | "copies" | "copy" | "focus" """

    def __init__(self, kind, shape, half=False):
        self.H = H = _native.hip()
        self.kind, self.half = kind, half
        dt, es = (np.float16, 2) if half else (np.float32, 4)
        x = np.random.default_rng(0).standard_normal(shape).astype(dt)
        self.c, self.pixels = shape[-1], int(np.prod(shape[:-1]))
        off = es if kind == "split_elem" else 0
        self.dx = DeviceBuffer(x.nbytes + 16)
        _chk(H.si_hip_memcpy_h2d(self.dx.ptr + off, x.ctypes.data_as(C.c_void_p), x.nbytes, None), "h2d")
        _chk(H.si_hip_stream_sync(None), "sync")
        self.px = self.dx.ptr + off
        self.bytes = 2 * x.nbytes
        tag = "%s %s" % ("fp16" if half else "fp32", "x".join(str(s) for s in shape))
        if kind in ("split", "split_elem", "copies"):
            k = len(SPLIT_WIDTHS)
            self.outs = [DeviceBuffer(self.pixels * w * es + 16) for w in SPLIT_WIDTHS]
            self.offsets = [sum(SPLIT_WIDTHS[:i]) for i in range(k)]
            ia = lambda v: (C.c_int * k)(*v)
            self.args = (self.px, self.pixels, self.c, self.c, k, ia(self.offsets), ia(SPLIT_WIDTHS),
                         (C.c_void_p * k)(*[b.ptr + off for b in self.outs]), ia(SPLIT_WIDTHS))
            if kind == "copies":
                self.kernel = "%d x copy_channels_kernel" % k
            else:
                self.kernel = H.si_hip_split_channels_kernel_name(*(self.args + (1 if half else 0,))).decode()
            self.fn = H.si_hip_split_channels_f16 if half else H.si_hip_split_channels_f32
            self.name = "split -> %s %s" % ("+".join(str(w) for w in SPLIT_WIDTHS), tag)
        elif kind == "copy":
            self.dy = DeviceBuffer(x.nbytes + 16)
            self.d = hipops.pad2d_desc(shape, (0, 0, 0, 0))
            self.kernel = H.si_hip_pad2d_kernel_name(C.byref(self.d), self.px, self.dy.ptr, 1 if half else 0).decode()
            self.fn = H.si_hip_pad2d_f16 if half else H.si_hip_pad2d_f32
            self.name = "copy %s" % tag
        else:
            self.descs = [hipops.slice_desc(shape, (ALL, slice(i, None, 2), slice(j, None, 2), ALL)) for i, j in ((0, 0), (1, 0), (0, 1), (1, 1))]
            self.outs = [DeviceBuffer(x.nbytes // 4 + 16) for _ in self.descs]
            self.kernel = "4 x " + H.si_hip_slice_kernel_name(C.byref(self.descs[0]), self.px, self.outs[0].ptr, 1 if half else 0).decode()
            self.fn = H.si_hip_slice_f16 if half else H.si_hip_slice_f32
            self.name = "focus slices %s" % tag

    def launch(self):
        H = self.H
        if self.kind in ("split", "split_elem"):
            _chk(self.fn(*(self.args + (None,))), self.name)
        elif self.kind == "copies":
            wd = 2 if self.half else 1       # fp16 travels as 4-byte words, as in Cat::Forward
            for off, w, out in zip(self.offsets, SPLIT_WIDTHS, self.outs):
                _chk(H.si_hip_copy_channels_f32(self.px + off * (2 if self.half else 4), self.pixels, w // wd, self.c // wd, out.ptr, w // wd, None), self.name)
        elif self.kind == "copy":
            _chk(self.fn(C.byref(self.d), self.px, self.dy.ptr, None), self.name)
        else:
            for d, out in zip(self.descs, self.outs):
                _chk(self.fn(C.byref(d), self.px, out.ptr, None), self.name)


class EngineCase:
    """one loaded engine of the C2f block; a launch is one forward, timed by the engine's own events"""

    def __init__(self, pp, bp, x, alias_split, half):
        self.e = Engine(alias_split=alias_split, fp16=1 if half else 0, graph=1, outputs_to_host=0, host_slices=1)
        self.e.load_model(pp, bp)
        self.e.input(self.e.input_names()[0], x)
        for _ in range(3):
            self.e.forward()
        step = [L for L in self.e.profile() if L["type"] == "torch.chunk"][0]
        self.kernel = "alias_split=%d: chunk step '%s', %d launches" % (alias_split, step["kernel"], len(self.e.schedule()["run"]))

    def ms(self, forwards):
        t = []
        for _ in range(forwards):
            self.e.forward()
            t.append(self.e.last_forward_ms())
        return float(np.median(t))


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


def compare(T, tags, cases, args):
    """alternating windows of the candidates; prints them and the ratios of each to the last one (the yardstick)"""
    for _ in range(2):   # warm-up
        for c in cases:
            T.window(c, 0.05)
    times = [[] for _ in cases]
    for _ in range(args.repeats):
        for c, t in zip(cases, times):
            t.append(T.window(c, args.seconds))
    med = [float(np.median(t)) for t in times]
    print(cases[0].name)
    for tag, c, t, m in zip(tags, cases, times, med):
        print("    %s [%-26s] %s ms   median %.4f ms  bytes / time %.2f TB/s = %.0f %% of %.1f  spread %.1f %%" % (
            tag, c.kernel, " ".join("%.4f" % v for v in t), m, c.bytes / m * 1e-9, 100 * c.bytes / m * 1e3 / HBM_BPS, HBM_BPS * 1e-12,
            100 * (max(t) - min(t)) / m))
    print("    " + "   ".join("%s / %s = %.3f" % (tag, tags[-1], m / med[-1]) for tag, m in zip(tags[:-1], med[:-1])) +
          ("   a / k = %.3f" % (med[0] / med[tags.index("k")]) if "k" in tags else ""), flush=True)


def engine_compare(args, half):
    b = mg.build_toy_c2f(args.batch, args.size, args.width, args.width, 2)
    x = mg.synth_input((args.batch, args.size, args.size, args.width))
    with tempfile.TemporaryDirectory() as td:
        pp, bp = os.path.join(td, "m.param"), os.path.join(td, "m.bin")
        b.save(pp, bp)
        engines = [EngineCase(pp, bp, x, 1, half), EngineCase(pp, bp, x, 0, half)]
        times = [[], []]
        for _ in range(args.repeats):
            for e, t in zip(engines, times):
                t.append(e.ms(args.forwards))
        med = [float(np.median(t)) for t in times]
        print("toy C2f %s: batch %d, %dx%d, %d -> %d channels, n = 2; median of %d forwards per window" % (
            "fp16 storage" if half else "fp32", args.batch, args.size, args.size, args.width, args.width, args.forwards))
        for e, t, m in zip(engines, times, med):
            print("    [%s] %s ms   median %.4f ms  spread %.1f %%" % (e.kernel, " ".join("%.4f" % v for v in t), m, 100 * (max(t) - min(t)) / m))
        print("    aliased / copied = %.3f" % (med[0] / med[1]), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--seconds", type=float, default=0.5)
    ap.add_argument("--forwards", type=int, default=200)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--size", type=int, default=80)
    ap.add_argument("--width", type=int, default=128)
    args = ap.parse_args()
    T = Timer()
    print("HIP-event windows >= %.2f s, %d alternating repeats.  kernel library: %s" % (args.seconds, args.repeats, _native.LIB_HIP_PATH))
    for half in (False, True):
        compare(T, "aekb", [Case(k, SPLIT_SHAPE, half) for k in ("split", "split_elem", "copies", "copy")], args)
    for half in (False, True):
        compare(T, "ab", [Case(k, FOCUS_SHAPE, half) for k in ("focus", "copy")], args)
    for half in (False, True):
        engine_compare(args, half)


if __name__ == "__main__":
    main()
