"""tools/bench_grid_sample.py -- speed of si_hip_grid_sample_f32 / _f16 (bilinear, border, align_corners=True) at batch 32 on 80x80x128 and
160x160x64 feature maps warped by a flow of a few pixels, output as large as the input.

Per shape and storage type, warmed up and then timed with HIP events over windows of >= --seconds, in turn, --repeats times in one process:
  a  the sampler reading the grid in place: the channels-first [N, 2, H, W] tensor stored NHWC, both coordinates in one load
  b  the sampler reading the rank-4 [N, H, W, 2] tensor as this project stores it ([N][W][2][H]: what a permute launch would have written;
     the permute itself is not in the figure)
  c  the sampler computing the coordinates from theta (F.affine_grid fused: the grid is never written)
  d  si_hip_affine_grid followed by the sampler on the stored grid it wrote (the two-launch path of c)
  y  the yardstick: si_hip_upsample_bilinear x2 writing the same output bytes (a bilinear gather with computed, perfectly regular taps)
Prints each window, the medians, the ratios a / y, b / y, b / a, d / c and the output bandwidth of each.
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
from tools.bench_deform_conv import Timer  # noqa: E402

N = 32
SHAPES = [(80, 80, 128), (160, 160, 64)]   # H, W, C


def base_grid(h, w):
    g = np.empty((N, h, w, 2), np.float32)
    g[..., 0] = np.linspace(-1, 1, w, dtype=np.float32)[None, None, :]
    g[..., 1] = np.linspace(-1, 1, h, dtype=np.float32)[None, :, None]
    return g


class Case:
    def __init__(self, kind, h, w, c, half):
        H = self.H = _native.hip()
        dt = np.float16 if half else np.float32
        rng = np.random.default_rng(0)
        self.kind, self.half = kind, half
        self.out_bytes = N * h * w * c * np.dtype(dt).itemsize
        self.dy = DeviceBuffer(self.out_bytes)
        sfx = "f16" if half else "f32"
        if kind == "y":
            x = rng.uniform(-1, 1, (N, h // 2, w // 2, c)).astype(dt)
            self.dx = DeviceBuffer.from_numpy(x)
            self.d = hipops.upsample_desc(x.shape, scale=2.0)
            self.fn = getattr(H, "si_hip_upsample_bilinear_" + sfx)
            self.name = H.si_hip_upsample_bilinear_kernel_name(C.byref(self.d), C.c_void_p(self.dx.ptr), C.c_void_p(self.dy.ptr), int(half)).decode()
            return
        x = rng.uniform(-1, 1, (N, h, w, c)).astype(dt)
        self.dx = DeviceBuffer.from_numpy(x)
        self.fn = getattr(H, "si_hip_grid_sample_" + sfx)
        if kind in ("c", "d"):
            theta = np.tile(np.asarray([[[0.96, 0.05, 0.01], [-0.05, 0.96, -0.02]]], np.float32), (N, 1, 1)).astype(dt)
            self.dt = DeviceBuffer.from_numpy(theta)
        if kind == "c":
            self.d = hipops.grid_sample_desc(x.shape, (h, w), "bilinear", "border", True, theta=True)
            self.dg = self.dt
        else:
            # a flow of up to +-2 px on top of the identity
            g = base_grid(h, w) + rng.uniform(-2, 2, (N, h, w, 2)).astype(np.float32) * np.asarray([2.0 / (w - 1), 2.0 / (h - 1)], np.float32)
            if kind == "a":
                img, strides = g.astype(dt), (h * w * 2, w * 2, 2, 1)
            else:
                img, strides = np.ascontiguousarray(g.transpose(0, 2, 3, 1)).astype(dt), (2 * w * h, 1, 2 * h, h)
            self.dg = DeviceBuffer.from_numpy(img)
            self.d = hipops.grid_sample_desc(x.shape, (h, w), "bilinear", "border", True, grid_strides=strides)
            if kind == "d":
                self.da = _native.SiAffineGridDesc(N, h, w, 0, 1)
                self.affine = getattr(H, "si_hip_affine_grid_" + sfx)
        self.name = H.si_hip_grid_sample_kernel_name(C.byref(self.d), C.c_void_p(self.dx.ptr), C.c_void_p(self.dg.ptr), C.c_void_p(self.dy.ptr), int(half)).decode()
        if kind == "d":
            self.name = "affine_grid + " + self.name

    def launch(self):
        if self.kind == "y":
            _chk(self.fn(C.byref(self.d), self.dx.ptr, self.dy.ptr, None), self.name)
            return
        if self.kind == "d":
            _chk(self.affine(C.byref(self.da), self.dt.ptr, self.dg.ptr, None), "affine_grid")
        _chk(self.fn(C.byref(self.d), self.dx.ptr, self.dg.ptr, self.dy.ptr, None), self.name)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--seconds", type=float, default=0.3)
    args = ap.parse_args()
    T = Timer()
    print("batch %d, bilinear / border / align_corners, HIP-event windows >= %.1f s, %d repeats in turn" % (N, args.seconds, args.repeats))
    kinds = ("a", "b", "c", "d", "y")
    for (h, w, c) in SHAPES:
        for half in (False, True):
            cases = {k: Case(k, h, w, c, half) for k in kinds}
            for k in kinds:
                T.window(cases[k], 0.05)
            t = {k: [] for k in kinds}
            for _ in range(args.repeats):
                for k in kinds:
                    t[k].append(T.window(cases[k], args.seconds)[0])
            m = {k: float(np.median(t[k])) for k in kinds}
            print("%dx%dx%d %s" % (h, w, c, "fp16" if half else "fp32"))
            for k in kinds:
                print("   %s %-52s %s ms   median %.4f ms, output %.2f TB/s" % (k, cases[k].name, " ".join("%.4f" % v for v in t[k]), m[k],
                                                                                cases[k].out_bytes / m[k] * 1e-9))
            print("   a / y = %.3f   b / y = %.3f   b / a = %.3f   c / a = %.3f   d / c = %.3f" % (m["a"] / m["y"], m["b"] / m["y"], m["b"] / m["a"],
                                                                                                    m["c"] / m["a"], m["d"] / m["c"]))
            del cases


if __name__ == "__main__":
    main()
