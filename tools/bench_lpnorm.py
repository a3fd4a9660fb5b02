"""tools/bench_lpnorm.py -- speed of the Lp-norm kernels (include/si_lpnorm.h) and of the planner pass fuse_norm, against code that already
exists and is not under test.

Shapes (file order): [32,256,60,80] (SuperPoint descriptors), [32,128,120,160], [4096,512], [256,2048]; p = 2 over dim 1; fp32 and fp16.
  1. op level, one process, alternating HIP-event windows of >= --seconds, --repeats repeats:
       n  si_hip_lpnorm, normalize = 1, eps = 0 (what the fused plan launches): one read and one write of the tensor, one IEEE division per element
       k  si_hip_param_act clamp on the same tensor: a pure one-read-one-write kernel
     bytes moved (read + write, counted from the shape) per second for both, and n / k.  Whether the per-element division keeps the fp16
     vector form bound by HBM rather than by the vector ALU is read off this ratio.
  2. through the engine: conv (or Linear) -> torch.norm -> [torch.unsqueeze] -> x / norm -> conv (or Linear), loaded twice, fuse_norm = 1 and
     fuse_norm = 0; the time of the norm / unsqueeze / div steps alone, from the engine's per-step events (Engine.profile), the median of
     --forwards forwards per window, the two engines alternating, --repeats windows each.  The layers around the pattern give it half operands
     under fp16 storage and are not counted.
Tensors below 256 MiB can live in the Infinity Cache, so bytes / time is not an HBM bandwidth there.
Run on an otherwise idle card, under a time limit:
  timeout -k 10 900 python tools/bench_lpnorm.py > profiles/lpnorm_<sha>.txt
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

SHAPES = [(32, 256, 60, 80), (32, 128, 120, 160), (4096, 512), (256, 2048)]
HBM_BPS = 8.0e12
PATTERN_TYPES = ("torch.norm", "torch.unsqueeze", "BinaryOp")


def nhwc(shape):
    return (shape[0], shape[2], shape[3], shape[1]) if len(shape) == 4 else (shape[0], 1, 1, shape[1])


class Case:
    """device operands and one launch of "normalize" | "clamp" on an NHWC tensor"""

    def __init__(self, kind, shape, half):
        self.H = H = _native.hip()
        dt = np.float16 if half else np.float32
        x = np.random.default_rng(0).standard_normal(shape).astype(dt)
        self.dx, self.dy = DeviceBuffer.from_numpy(x), DeviceBuffer(x.nbytes + 16)
        self.bytes = 2 * x.nbytes
        self.name = "%s %s" % ("fp16" if half else "fp32", "x".join(str(s) for s in shape))
        if kind == "normalize":
            self.d = hipops.lpnorm_desc(shape, 2, 8, True, 0.0)
            self.kernel = H.si_hip_lpnorm_kernel_name(C.byref(self.d), self.dx.ptr, self.dy.ptr, 1 if half else 0).decode()
            self.fn = H.si_hip_lpnorm_f16 if half else H.si_hip_lpnorm_f32
        else:
            self.d = hipops.param_act_desc(shape, "clamp", -1.0, 1.0)
            self.kernel = H.si_hip_param_act_kernel_name(C.byref(self.d), self.dx.ptr, self.dy.ptr, 1 if half else 0).decode()
            self.fn = H.si_hip_param_act_f16 if half else H.si_hip_param_act_f32

    def launch(self):
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


def op_level(T, shape, half, args):
    cases = [Case("normalize", shape, half), Case("clamp", shape, half)]
    for _ in range(2):   # warm-up
        for c in cases:
            T.window(c, 0.02)
    times = [[] for _ in cases]
    for _ in range(args.repeats):
        for c, t in zip(cases, times):
            t.append(T.window(c, args.seconds))
    med = [float(np.median(t)) for t in times]
    print("op level, %s" % cases[0].name)
    for tag, c, t, m in zip("nk", cases, times, med):
        print("    %s [%-40s] %s ms   median %.4f ms  bytes moved / time %.2f TB/s = %.0f %% of %.1f  spread %.1f %%" % (
            tag, c.kernel, " ".join("%.4f" % v for v in t), m, c.bytes / m * 1e-9, 100 * c.bytes / m * 1e3 / HBM_BPS, HBM_BPS * 1e-12,
            100 * (max(t) - min(t)) / m))
    print("    n / k = %.3f" % (med[0] / med[1]), flush=True)
    return med[0] / med[1]


def pattern_graph(shape):
    """conv 1x1 (rank 4) or Linear (rank 2) -> the written-out normalisation over dim 1 -> the same layer again"""
    b = mg.PnnxBuilder(seed=1)
    x = b.input(shape)
    layer = (lambda v: b.conv(v, shape[1], 1)) if len(shape) == 4 else (lambda v: b.linear(v, shape[1]))
    f = layer(x)
    if len(shape) == 4:
        q = b.div(f, b.unsqueeze(b.norm(f, 1, 2, False), 1))
    else:
        q = b.div(f, b.norm(f, 1, 2, True))      # (the rank-1 result of keepdim=False is not served)
    b.output(layer(q))
    return b


class EngineCase:
    def __init__(self, pp, bp, x, fuse_norm, half):
        self.e = Engine(fuse_norm=fuse_norm, fp16=1 if half else 0, outputs_to_host=0, host_slices=1)
        self.e.load_model(pp, bp)
        self.e.input(self.e.input_names()[0], x)
        for _ in range(2):
            self.e.forward()
        steps = [L for L in self.e.profile() if L["type"] in PATTERN_TYPES]
        self.what = "fuse_norm=%d: %s" % (fuse_norm, " + ".join("%s '%s'" % (L["type"], L["kernel"]) for L in steps))

    def ms(self, forwards):
        t = []
        for _ in range(forwards):
            t.append(sum(L["ms"] for L in self.e.profile() if L["type"] in PATTERN_TYPES))
        return float(np.median(t))


def engine_level(shape, half, args):
    b = pattern_graph(shape)
    x = mg.synth_input(nhwc(shape) if len(shape) == 4 else shape)
    with tempfile.TemporaryDirectory() as td:
        pp, bp = os.path.join(td, "m.param"), os.path.join(td, "m.bin")
        b.save(pp, bp)
        engines = [EngineCase(pp, bp, x, 1, half), EngineCase(pp, bp, x, 0, half)]
        times = [[], []]
        for _ in range(args.repeats):
            for e, t in zip(engines, times):
                t.append(e.ms(args.forwards))
    med = [float(np.median(t)) for t in times]
    print("engine, %s %s: the norm / unsqueeze / div steps, median of %d forwards per window" % (
        "fp16 storage" if half else "fp32", "x".join(map(str, shape)), args.forwards))
    for e, t, m in zip(engines, times, med):
        print("    [%s] %s ms   median %.4f ms  spread %.1f %%" % (e.what, " ".join("%.4f" % v for v in t), m, 100 * (max(t) - min(t)) / max(m, 1e-9)))
    print("    fused / unfused = %.3f" % (med[0] / med[1]), flush=True)
    return med[0] / med[1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--seconds", type=float, default=0.2)
    ap.add_argument("--forwards", type=int, default=10)
    ap.add_argument("--shapes", type=int, default=len(SHAPES), help="the first k shapes only")
    args = ap.parse_args()
    T = Timer()
    print("HIP-event windows >= %.2f s, %d alternating repeats.  kernel library: %s" % (args.seconds, args.repeats, os.path.relpath(_native.LIB_HIP_PATH, ROOT)))
    summary = []
    for shape in SHAPES[:args.shapes]:
        for half in (False, True):
            r_op = op_level(T, nhwc(shape), half, args)
            r_en = engine_level(shape, half, args)
            summary.append(("x".join(map(str, shape)), "fp16" if half else "fp32", r_op, r_en))
    print("summary: shape, storage, normalize / clamp (op level), fused / unfused (engine steps)")
    for row in summary:
        print("    %-16s %s  %.3f  %.3f" % row)


if __name__ == "__main__":
    main()
