"""tools/bench_layernorm.py -- speed of the layer-norm kernels (include/si_layernorm.h) against code that already exists and is not under test.

Shapes [rows, c]: [32*196, 384], [32*400, 256], [8*1024, 768], [64, 4096], [64, 8192]; weight and bias given; fp32 and fp16.
One process, alternating windows of >= --seconds, --repeats repeats, medians:
    l  si_hip_layernorm: one read and one write of the tensor (three reads in the 3-pass form), gamma / beta once per workgroup
    k  si_hip_param_act clamp on the same tensor: a pure one-read-one-write kernel, the project's HBM-bound yardstick
    t  the installed torch's F.layer_norm on the same values (torch.cuda events; its own allocation)
l and k are timed with HIP events, bytes moved (read + write, counted from the shape) per second, and l / k, l / t are printed.
Tensors below 256 MiB can live in the Infinity Cache, so bytes / time is not an HBM bandwidth there; the two small shapes are launch-bound.
Run on an otherwise idle card, under a time limit:
  timeout -k 10 600 python tools/bench_layernorm.py > profiles/layernorm_<sha>.txt
"""
import argparse
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from simpleinfer_amd import _native, hipops  # noqa: E402
from simpleinfer_amd.hipops import DeviceBuffer, _chk  # noqa: E402
from bench_lpnorm import HBM_BPS, Timer  # noqa: E402

SHAPES = [(32 * 196, 384), (32 * 400, 256), (8 * 1024, 768), (64, 4096), (64, 8192)]


class Case:
    """device operands and one launch of "layernorm" | "clamp" on a [rows, c] tensor"""

    def __init__(self, kind, x):
        self.H = H = _native.hip()
        half = x.dtype == np.float16
        rows, c = x.shape
        self.dx, self.dy = DeviceBuffer.from_numpy(x), DeviceBuffer(x.nbytes + 16)
        self.bytes = 2 * x.nbytes
        self.name = "%s %dx%d" % ("fp16" if half else "fp32", rows, c)
        if kind == "layernorm":
            r = np.random.default_rng(1)
            self.dg = DeviceBuffer.from_numpy(r.uniform(0.5, 1.5, c).astype(np.float32))
            self.db = DeviceBuffer.from_numpy(r.uniform(-0.5, 0.5, c).astype(np.float32))
            self.d = hipops.layernorm_desc(rows, c)
            self.kernel = H.si_hip_layernorm_kernel_name(C.byref(self.d), self.dx.ptr, self.dy.ptr, 1 if half else 0).decode()
            fn = H.si_hip_layernorm_f16 if half else H.si_hip_layernorm_f32
            self.call = lambda: fn(C.byref(self.d), self.dx.ptr, self.dg.ptr, self.db.ptr, self.dy.ptr, None)
        else:
            self.d = hipops.param_act_desc(x.shape, "clamp", -1.0, 1.0)
            self.kernel = H.si_hip_param_act_kernel_name(C.byref(self.d), self.dx.ptr, self.dy.ptr, 1 if half else 0).decode()
            fn = H.si_hip_param_act_f16 if half else H.si_hip_param_act_f32
            self.call = lambda: fn(C.byref(self.d), self.dx.ptr, self.dy.ptr, None)

    def launch(self):
        _chk(self.call(), self.name)


class TorchCase:
    """torch's own F.layer_norm on its own copy of the values; window(): mean ms per call over >= seconds, by torch.cuda events"""

    def __init__(self, x):
        import torch
        self.torch = torch
        c = x.shape[1]
        self.x = torch.from_numpy(x).cuda()
        self.g, self.b = torch.ones(c, device="cuda", dtype=self.x.dtype), torch.zeros(c, device="cuda", dtype=self.x.dtype)
        self.kernel = "torch %s F.layer_norm" % torch.__version__
        self.bytes = 2 * x.nbytes

    def time(self, iters):
        torch = self.torch
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            torch.nn.functional.layer_norm(self.x, (self.x.shape[1],), self.g, self.b, 1e-5)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    def window(self, seconds):
        est = self.time(10) / 10
        iters = max(20, int(seconds * 1000.0 / max(est, 1e-3)) + 1)
        return self.time(iters) / iters


def one_shape(T, shape, half, args):
    x = (3.0 + 0.5 * np.random.default_rng(0).standard_normal(shape)).astype(np.float16 if half else np.float32)
    cases = [Case("layernorm", x), Case("clamp", x)]
    tc = TorchCase(x)
    for _ in range(2):   # warm-up
        for c in cases:
            T.window(c, 0.02)
        tc.window(0.02)
    times = [[], [], []]
    for _ in range(args.repeats):
        for c, t in zip(cases, times):
            t.append(T.window(c, args.seconds))
        times[2].append(tc.window(args.seconds))
    med = [float(np.median(t)) for t in times]
    print(cases[0].name)
    for tag, c, t, m in zip("lkt", cases + [tc], times, med):
        print("    %s [%-44s] %s ms   median %.4f ms  bytes moved / time %.2f TB/s = %.0f %% of %.1f  spread %.1f %%" % (
            tag, c.kernel, " ".join("%.4f" % v for v in t), m, c.bytes / m * 1e-9, 100 * c.bytes / m * 1e3 / HBM_BPS, HBM_BPS * 1e-12,
            100 * (max(t) - min(t)) / m))
    print("    l / k = %.3f   l / t = %.3f" % (med[0] / med[1], med[0] / med[2]), flush=True)
    return med[0] / med[1], med[0] / med[2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--seconds", type=float, default=0.2)
    args = ap.parse_args()
    T = Timer()
    print("windows >= %.2f s, %d alternating repeats.  kernel library: %s" % (args.seconds, args.repeats, os.path.relpath(_native.LIB_HIP_PATH, ROOT)))
    summary = []
    for shape in SHAPES:
        for half in (False, True):
            summary.append(("%dx%d" % shape, "fp16" if half else "fp32") + one_shape(T, shape, half, args))
    print("summary: shape, storage, layernorm / clamp, layernorm / torch")
    for row in summary:
        print("    %-12s %s  %.3f  %.3f" % row)


if __name__ == "__main__":
    main()
