"""tools/bench_border.py -- the one-launch border-mapped convolution (include/si_border.h) against the composition it replaces:
si_hip_pad2d_* into a padded tensor, then si_hip_conv2d_f32 / si_hip_conv2d_f16 with zero padding over it -- what a layer with
padding_mode = reflect | replicate | circular costs on either path, on the same data.

Default run: per shape and storage type the candidate (a: one launch) and the composition (b: two launches) are warmed up, then timed with
HIP events over windows of >= --seconds, a then b, --repeats times in one process.  Prints each window, the medians, their ratio and the
spread; "bytes / time" counts a's compulsory traffic (x read, y written, weights read) and, for b, the padded tensor's round trip on top.
Nothing here is an acceptance criterion: the table decides which path a shape class takes.
  shapes (n, h, w, ic, oc, k, pad, dilation, mode): a residual-block layer, a high-resolution layer, a 7x7 stem-like layer, a dilated layer; three thin layers.
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

SHAPES = [(8, 64, 64, 256, 256, 3, 1, 1, "reflect"), (1, 512, 512, 64, 64, 3, 1, 1, "replicate"), (4, 128, 128, 64, 64, 7, 3, 1, "reflect"),
          (4, 64, 64, 128, 128, 3, 2, 2, "circular"),
          # thin layers, below the 64 input channels of the shapes above: a generator's RGB stem (fp32 only: ic % 8 != 0) and its narrow blocks
          (4, 256, 256, 3, 32, 7, 3, 1, "reflect"), (8, 128, 128, 32, 32, 3, 1, 1, "reflect"), (8, 64, 64, 16, 16, 3, 1, 1, "replicate")]


class Case:
    """device operands and one run of: "border" (one launch) | "composed" (pad, then the zero-pad convolution)"""

    def __init__(self, kind, n, h, w, ic, oc, k, pad, dil, mode, half=False):
        H = self.H = _native.hip()
        self.kind, self.half = kind, half
        dt = np.float16 if half else np.float32
        r = np.random.default_rng(0)
        x = r.standard_normal((n, h, w, ic)).astype(dt)
        wt = (r.standard_normal((oc, ic, k, k)) / np.sqrt(ic * k * k)).astype(np.float32)
        self.dx, self.db = DeviceBuffer.from_numpy(x), DeviceBuffer.from_numpy(np.zeros(oc, np.float32))
        self.d = hipops.conv2d_border_desc(x.shape, wt.shape, (1, 1), (pad, pad), (dil, dil), mode, act1="relu")
        oh, ow = self.d.oh, self.d.ow
        self.dy = DeviceBuffer(n * oh * ow * oc * x.itemsize)
        padded = n * (h + 2 * pad) * (w + 2 * pad) * ic * x.itemsize
        self.bytes = x.nbytes + n * oh * ow * oc * x.itemsize + wt.size * x.itemsize + (2 * padded if kind == "composed" else 0)
        wp = wt.ctypes.data_as(C.c_void_p)
        if kind == "border":
            packed = np.zeros(H.si_hip_conv2d_border_weight_elems(C.byref(self.d), int(half)), dt)
            _chk(H.si_hip_conv2d_border_pack_weight_host(C.byref(self.d), wp, packed.ctypes.data_as(C.c_void_p), int(half)), "pack")
            kernel = H.si_hip_conv2d_border_kernel_name(C.byref(self.d), self.dx.ptr, self.dy.ptr, int(half)).decode()
        else:
            self.pd = hipops.pad2d_desc(x.shape, (pad,) * 4, mode)
            self.dp = DeviceBuffer(padded)
            self.cd = hipops.SiConv2dDesc(n, h + 2 * pad, w + 2 * pad, ic, ic, oh, ow, oc, oc, k, k, 1, 1, dil, dil, 0, 0, 1, 1, hipops.ACT["relu"], 0, oc, 0, 0.0)
            elems, pack = (H.si_hip_conv2d_f16_weight_elems, H.si_hip_conv2d_f16_pack_weight_host) if half else (
                H.si_hip_conv2d_weight_elems, H.si_hip_conv2d_pack_weight_host)
            packed = np.zeros(elems(C.byref(self.cd)), dt)
            _chk(pack(C.byref(self.cd), wp, packed.ctypes.data_as(C.c_void_p)), "pack")
            kernel = "pad2d + " + (H.si_hip_conv2d_f16_kernel_name(C.byref(self.cd), 0) if half else H.si_hip_conv2d_kernel_name(C.byref(self.cd), self.dp.ptr)).decode()
        self.dw = DeviceBuffer.from_numpy(packed)
        self.name = "%s %s %dx%dx%dx%d->%d k%d p%d d%d %s [%s]" % (kind, "fp16" if half else "fp32", n, h, w, ic, oc, k, pad, dil, mode, kernel)

    def launch(self):
        H = self.H
        if self.kind == "border":
            fn = H.si_hip_conv2d_border_f16 if self.half else H.si_hip_conv2d_border_f32
            _chk(fn(C.byref(self.d), self.dx.ptr, self.dw.ptr, self.db.ptr, None, self.dy.ptr, None), self.name)
            return
        _chk((H.si_hip_pad2d_f16 if self.half else H.si_hip_pad2d_f32)(C.byref(self.pd), self.dx.ptr, self.dp.ptr, None), self.name)
        if self.half:
            _chk(H.si_hip_conv2d_f16(C.byref(self.cd), self.dp.ptr, self.dw.ptr, self.db.ptr, None, self.dy.ptr, 0, None), self.name)
        else:
            _chk(H.si_hip_conv2d_f32(C.byref(self.cd), self.dp.ptr, self.dw.ptr, self.db.ptr, None, self.dy.ptr, None), self.name)


def cases():
    for half in (False, True):
        for s in SHAPES:
            if half and s[3] % 8 != 0:
                continue
            yield Case("border", *s, half=half), Case("composed", *s, half=half), None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--profile", action="store_true")
    args = ap.parse_args()
    if args.profile:
        for a, b, _ in cases():
            for _ in range(20):
                a.launch()
                b.launch()
            _chk(_native.hip().si_hip_device_sync(), "sync")
        print("profile: 20 launches of every candidate and composition")
        return
    T = Timer()
    print("HIP-event windows >= %.1f s, %d alternating repeats (a = one launch, b = pad2d + zero-pad conv)" % (args.seconds, args.repeats))
    rows = []
    for a, b, bar in cases():
        rows.append((a.name, compare(T, a, b, args, bar)))
    for name, r in rows:
        print("a/b = %.3f  %s" % (r, name))


if __name__ == "__main__":
    main()
