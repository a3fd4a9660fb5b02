"""tools/bench_roi_align.py -- speed of si_hip_roi_align_f32 / _f16: K = 512 and 1000 boxes of FPN-like sizes on two levels of one 800 x 1088
image with 256 channels -- 200x272 (stride 4, boxes of 32 .. 112 px) and 50x68 (stride 16, boxes of 224 .. 448 px) --, outputs 7x7 and 14x14,
sampling_ratio 2 and adaptive (0).

Per case, warmed up and then timed with HIP events over windows of >= --seconds, in turn, --repeats times in one process.  Beside every
(K, output, type): two yardsticks writing the same number of output bytes in the same run -- u: si_hip_upsample_bilinear x2, g: si_hip_grid_sample
(bilinear, border, the dense grid of a +-2 px flow), both on [1, K / 2, ph pw, 128] -> [1, K, 2 ph pw, 128].
Prints each window, the medians in us, the output bandwidth, the bilinear samples per output element (counted on the host from the boxes, by the
rule's own float32 arithmetic) and the time per sample and element, and the ratios to the yardsticks.
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

CH = 256
IMAGE = (800, 1088)
LEVELS = [(200, 272, 0.25, (32.0, 112.0)), (50, 68, 0.0625, (224.0, 448.0))]   # h, w, spatial_scale, box sizes in image pixels
N = 2


def boxes(k, lo, hi, seed):
    rng = np.random.default_rng(seed)
    bw, bh = rng.uniform(lo, hi, k), rng.uniform(lo, hi, k)
    cx, cy = rng.uniform(0, IMAGE[1], k), rng.uniform(0, IMAGE[0], k)
    r = np.stack([rng.integers(0, N, k), cx - bw / 2, cy - bh / 2, cx + bw / 2, cy + bh / 2], 1)
    return r.astype(np.float32)


def samples_per_element(rois, out, scale, ratio):
    """mean over the boxes of gh * gw, in the rule's float32 arithmetic (aligned=False)"""
    f = np.float32
    rw = np.maximum(rois[:, 3] * f(scale) - rois[:, 1] * f(scale), f(1))
    rh = np.maximum(rois[:, 4] * f(scale) - rois[:, 2] * f(scale), f(1))
    if ratio > 0:
        return float(ratio * ratio)
    return float(np.mean(np.ceil(rh / f(out)) * np.ceil(rw / f(out))))


class RoiCase:
    def __init__(self, level, k, out, half, ratio):
        H = self.H = _native.hip()
        h, w, scale, (lo, hi) = level
        dt = np.float16 if half else np.float32
        x = np.random.default_rng(0).uniform(-1, 1, (N, h, w, CH)).astype(dt)
        rois = boxes(k, lo, hi, 1)
        self.dx, self.dr = DeviceBuffer.from_numpy(x), DeviceBuffer.from_numpy(rois)
        self.out_bytes = k * out * out * CH * np.dtype(dt).itemsize
        self.dy = DeviceBuffer(self.out_bytes)
        self.d = hipops.roi_align_desc(x.shape, k, out, scale, ratio, False)
        self.fn = getattr(H, "si_hip_roi_align_" + ("f16" if half else "f32"))
        self.name = H.si_hip_roi_align_kernel_name(C.byref(self.d), C.c_void_p(self.dx.ptr), C.c_void_p(self.dr.ptr), C.c_void_p(self.dy.ptr), int(half)).decode()
        self.samples = samples_per_element(rois, out, scale, ratio)

    def launch(self):
        _chk(self.fn(C.byref(self.d), self.dx.ptr, self.dr.ptr, self.dy.ptr, None), self.name)


class Yardstick:
    """u: bilinear x2 upsample, g: grid_sample; [1, K / 2, ph pw, 128] -> [1, K, 2 ph pw, 128]: the output bytes of RoiCase(k, out)"""

    def __init__(self, kind, k, out, half):
        H = self.H = _native.hip()
        dt = np.float16 if half else np.float32
        sfx = "f16" if half else "f32"
        ih, iw, c = k // 2, out * out, CH // 2
        rng = np.random.default_rng(0)
        x = rng.uniform(-1, 1, (1, ih, iw, c)).astype(dt)
        self.kind = kind
        self.dx = DeviceBuffer.from_numpy(x)
        self.out_bytes = 4 * x.size * np.dtype(dt).itemsize
        self.dy = DeviceBuffer(self.out_bytes)
        self.samples = 1.0
        if kind == "u":
            self.d = hipops.upsample_desc(x.shape, scale=2.0)
            self.fn = getattr(H, "si_hip_upsample_bilinear_" + sfx)
            self.name = H.si_hip_upsample_bilinear_kernel_name(C.byref(self.d), C.c_void_p(self.dx.ptr), C.c_void_p(self.dy.ptr), int(half)).decode()
            return
        oh, ow = 2 * ih, 2 * iw
        g = np.empty((1, oh, ow, 2), np.float32)
        g[..., 0] = np.linspace(-1, 1, ow, dtype=np.float32)[None, None, :]
        g[..., 1] = np.linspace(-1, 1, oh, dtype=np.float32)[None, :, None]
        g += rng.uniform(-2, 2, g.shape).astype(np.float32) * np.asarray([2.0 / (ow - 1), 2.0 / (oh - 1)], np.float32)
        self.dg = DeviceBuffer.from_numpy(g.astype(dt))
        self.d = hipops.grid_sample_desc(x.shape, (oh, ow), "bilinear", "border", True)
        self.fn = getattr(H, "si_hip_grid_sample_" + sfx)
        self.name = H.si_hip_grid_sample_kernel_name(C.byref(self.d), C.c_void_p(self.dx.ptr), C.c_void_p(self.dg.ptr), C.c_void_p(self.dy.ptr), int(half)).decode()

    def launch(self):
        if self.kind == "u":
            _chk(self.fn(C.byref(self.d), self.dx.ptr, self.dy.ptr, None), self.name)
        else:
            _chk(self.fn(C.byref(self.d), self.dx.ptr, self.dg.ptr, self.dy.ptr, None), self.name)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--seconds", type=float, default=0.2)
    args = ap.parse_args()
    T = Timer()
    print("%d channels, %d images, aligned=False, HIP-event windows >= %.1f s, %d repeats in turn" % (CH, N, args.seconds, args.repeats))
    for k in (512, 1000):
        for out in (7, 14):
            for half in (False, True):
                cases = {"u": Yardstick("u", k, out, half), "g": Yardstick("g", k, out, half)}
                for li, level in enumerate(LEVELS):
                    for ratio in (2, 0):
                        cases["L%d r%d" % (li, ratio)] = RoiCase(level, k, out, half, ratio)
                for c in cases.values():
                    T.window(c, 0.03)
                t = {key: [] for key in cases}
                for _ in range(args.repeats):
                    for key, c in cases.items():
                        t[key].append(T.window(c, args.seconds)[0])
                m = {key: float(np.median(v)) for key, v in t.items()}
                print("K %d, %dx%d, %s: %.1f MB of output" % (k, out, out, "fp16" if half else "fp32", cases["u"].out_bytes * 1e-6))
                for key, c in cases.items():
                    level = "" if key in "ug" else "  map %dx%d ratio %s" % (LEVELS[int(key[1])][0], LEVELS[int(key[1])][1], "adaptive" if key.endswith("r0") else "2")
                    print("   %-6s %-44s %s us   median %8.2f us, output %5.2f TB/s, %5.2f samples / element, %6.3f ns / (sample x MB)  u x %.2f  g x %.2f%s" % (
                        key, c.name, " ".join("%8.2f" % (v * 1e3) for v in t[key]), m[key] * 1e3, c.out_bytes / m[key] * 1e-9, c.samples,
                        m[key] * 1e6 / (c.samples * c.out_bytes * 1e-6), m[key] / m["u"], m[key] / m["g"], level))
                del cases


if __name__ == "__main__":
    main()
