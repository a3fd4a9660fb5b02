"""tools/bench_pad.py -- speed of si_hip_pad2d_f32 / _f16 (batch 8).

Default run: per shape the candidate (a) and its yardstick (b) -- si_hip_copy_channels_f32 over the n * oh * ow pixels of c channels of
the OUTPUT: one read plus one write of the output's size, which the pad must at least move; for fp16 the copy kernel called with c / 2
words, as the Upsample layer calls the nearest kernel (c odd: two pixels as one of c words) -- are warmed up, then timed with HIP
events over windows of >= 1 s, a then b, --repeats times in one process.  Prints each window, the medians, their ratio and the spread.
Bytes are counted from shapes (a: n ih iw c read + n oh ow c written; b: n oh ow c both ways); "bytes / time" is printed next to the
6.3 TB/s achievable HBM bandwidth, but these tensors fit the 256 MiB Infinity Cache, so it is not an HBM bandwidth.
  shapes (ih, iw, c, pad, mode): the RGB stem, the residual-block pad (two per block), a wider map, a zero pad.  Expectation, not a
  test: a <= 1.25 b, the project's bar for copy-class kernels (tools/bench_upsample.py).
--profile: launches every case a few times (for a rocprofv3 --kernel-trace --stats run of its own).
--model: the per-layer profile of build_toy_cyclegan(--model-batch, --model-size, --model-base, --model-blocks) summed by operator type:
the share of the pad launches in the whole generator.
"""
import argparse
import ctypes as C
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_upsample import Timer, compare  # noqa: E402
from simpleinfer_amd import _native, hipops  # noqa: E402
from simpleinfer_amd.hipops import DeviceBuffer, _chk  # noqa: E402

N = 8
SHAPES = [(256, 256, 3, 3, "reflect"), (64, 64, 256, 1, "reflect"), (128, 128, 128, 1, "reflect"), (64, 64, 256, 1, "constant")]
BAR = 1.25


class Case:
    """device operands and one launch of: "pad" | "copy" (the yardstick)"""

    def __init__(self, kind, ih, iw, c, pad, mode, half=False):
        self.H = _native.hip()
        self.kind, self.half, self.c = kind, half, c
        dt = np.float16 if half else np.float32
        x = np.random.default_rng(0).standard_normal((N, ih, iw, c)).astype(dt)
        self.d = hipops.pad2d_desc(x.shape, (pad,) * 4, mode)
        self.out_px = N * self.d.oh * self.d.ow
        out_bytes = self.out_px * c * x.itemsize
        if kind == "pad":
            self.dx = DeviceBuffer.from_numpy(x)
            self.bytes = x.nbytes + out_bytes
        else:
            self.dx = DeviceBuffer(out_bytes)
            self.dx.fill(0)
            self.bytes = 2 * out_bytes
        self.dy = DeviceBuffer(out_bytes)
        self.name = "%s %s %dx%dx%d pad %d %s" % (kind, "fp16" if half else "fp32", ih, iw, c, pad, mode)
        if kind == "pad":
            self.name += " [%s]" % self.H.si_hip_pad2d_kernel_name(C.byref(self.d), self.dx.ptr, self.dy.ptr, 1 if half else 0).decode()

    def launch(self):
        H = self.H
        if self.kind == "pad":
            fn = H.si_hip_pad2d_f16 if self.half else H.si_hip_pad2d_f32
            rc = fn(C.byref(self.d), self.dx.ptr, self.dy.ptr, None)
        else:
            # (fp16: pure data movement as 4-byte words; an odd c: two pixels travel as one of c words)
            px, words = self.out_px, self.c
            if self.half:
                px, words = (px, self.c // 2) if self.c % 2 == 0 else (px // 2, self.c)
            rc = H.si_hip_copy_channels_f32(self.dx.ptr, px, words, words, self.dy.ptr, words, None)
        _chk(rc, self.name)


def cases():
    for half in (False, True):
        for ih, iw, c, pad, mode in SHAPES:
            yield Case("pad", ih, iw, c, pad, mode, half), Case("copy", ih, iw, c, pad, mode, half), BAR


def model_profile(args):
    from simpleinfer_amd import modelgen as mg
    from simpleinfer_amd.engine import Engine
    b = mg.build_toy_cyclegan(batch=args.model_batch, size=args.model_size, base=args.model_base, blocks=args.model_blocks)
    x = mg.synth_input((args.model_batch, args.model_size, args.model_size, 3))
    with tempfile.TemporaryDirectory() as tmp:
        pp, bp = os.path.join(tmp, "g.pnnx.param"), os.path.join(tmp, "g.pnnx.bin")
        b.save(pp, bp)
        for opts in ({}, dict(fp16=1)):
            e = Engine(**opts)
            e.load_model(pp, bp)
            e.input(e.input_names()[0], x)
            for _ in range(3):
                e.forward()
            tot = {}
            for _ in range(args.model_runs):   # profile(): one timed run of every layer; the median of a few
                for L in e.profile():
                    tot.setdefault((L["type"], L["kernel"]), []).append((L["name"], L["ms"]))
            rows = {}
            for (typ, kernel), v in tot.items():
                names = sorted({n for n, _ in v})
                ms = sum(float(np.median([t for n2, t in v if n2 == n])) for n in names)
                rows[(typ, kernel)] = (len(names), ms)
            whole = sum(ms for _, ms in rows.values())
            print("build_toy_cyclegan(batch=%d, size=%d, base=%d, blocks=%d) %s: %d layers, sum of layer times %.3f ms" % (
                args.model_batch, args.model_size, args.model_base, args.model_blocks, "fp16 storage" if opts else "fp32",
                sum(n for n, _ in rows.values()), whole))
            for (typ, kernel), (n, ms) in sorted(rows.items(), key=lambda kv: -kv[1][1]):
                print("    %-22s x%-3d %8.3f ms  %5.1f %%  %s" % (typ, n, ms, 100 * ms / whole, kernel))
            pads = sum(ms for (typ, _), (_, ms) in rows.items() if "Pad" in typ or typ == "F.pad")
            print("    explicit pads: %.3f ms = %.1f %% of the sum" % (pads, 100 * pads / whole))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--model", action="store_true")
    ap.add_argument("--model-batch", type=int, default=1)
    ap.add_argument("--model-size", type=int, default=256)
    ap.add_argument("--model-base", type=int, default=64)
    ap.add_argument("--model-blocks", type=int, default=9)
    ap.add_argument("--model-runs", type=int, default=5)
    args = ap.parse_args()
    if args.model:
        model_profile(args)
        return
    if args.profile:
        for a, b, _ in cases():
            for _ in range(20):
                a.launch()
                b.launch()
            _chk(_native.hip().si_hip_device_sync(), "sync")
        print("profile: 20 launches of every candidate and yardstick")
        return
    T = Timer()
    print("batch %d, HIP-event windows >= %.1f s, %d alternating repeats (a = candidate, b = si_hip_copy_channels_f32 over the output's bytes)" %
          (N, args.seconds, args.repeats))
    worst, missed = 0.0, []
    for a, b, bar in cases():
        r = compare(T, a, b, args, bar)
        worst = max(worst, r)
        if r > bar:
            missed.append(a.name)
    print("worst a/b = %.3f (expectation %.2f); above it: %s" % (worst, BAR, ", ".join(missed) if missed else "none"))


if __name__ == "__main__":
    main()
