"""tools/bench_conv1d.py -- speed of the temporal convolution kernels (include/si_conv1d.h) against the code they replace.

Shapes at batch 32, L = 500, fp32 and fp16 storage: dense 64 -> 256 K = 33 stride 2; pointwise 256 -> 256 and 512 -> 512; TCN 128 -> 128 K = 3
with dilation 1 and 64; depthwise C = 256 K = 33 and C = 512 K = 75.  Per shape, the candidates timed in one process in alternating windows:
  a  si_hip_conv1d_*   on [N, C, L], the native layout
  b  si_hip_conv2d_*   on the [N, 1, L, C] image of the same problem (what a graph would run if its tensors already were NHWC)
  p  the same conv2d between the two permute_tile launches a graph needs ([N, C, L] -> [N, L, C] in front, [N, Lo, OC] -> [N, OC, Lo] behind)
  c  depthwise only: si_hip_copy_channels_f32 moving the bytes the depthwise kernel moves (one read of x, one write of y)
Windows of >= --seconds, --repeats alternating repeats; prints each candidate's median, the spread of its windows, the FLOP rate counted from
the shapes and the ratios a / b and a / p (below 1: the new kernel is faster).  A candidate the fp16 conv2d does not serve is left out.
Run on an otherwise idle card under a time limit:
  timeout -k 10 600 python tools/bench_conv1d.py > profiles/conv1d_<sha>.txt
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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_layout import Timer  # noqa: E402

# (name, C, OC, K, stride, pad, dilation, groups)
SHAPES = [("dense 64->256 K33 s2", 64, 256, 33, 2, 16, 1, 1), ("pointwise 256->256", 256, 256, 1, 1, 0, 1, 1), ("pointwise 512->512", 512, 512, 1, 1, 0, 1, 1),
          ("tcn 128->128 K3 d1", 128, 128, 3, 1, 1, 1, 1), ("tcn 128->128 K3 d64", 128, 128, 3, 1, 64, 64, 1),
          ("depthwise 256 K33", 256, 256, 33, 1, 16, 1, 256), ("depthwise 512 K75", 512, 512, 75, 1, 37, 1, 512)]


class Problem:
    """one shape in one storage type: the buffers and weight images every candidate shares"""

    def __init__(self, shape, n, l, half):
        self.H = H = _native.hip()
        self.name, self.c, self.oc, self.k, self.s, self.p, self.d, self.g = shape
        self.n, self.l, self.half = n, l, half
        self.lo = hipops.conv1d_out_len(l, self.k, self.s, self.p, self.d)
        es = 2 if half else 4
        dt = np.float16 if half else np.float32
        r = np.random.Generator(np.random.Philox(1))
        self.x = DeviceBuffer.from_numpy(r.uniform(-1, 1, (n, self.c, l)).astype(dt))
        self.xt = DeviceBuffer(n * self.c * l * es)            # [N, L, C]
        self.y = DeviceBuffer(n * self.oc * self.lo * es)
        self.yt = DeviceBuffer(n * self.oc * self.lo * es)     # [N, Lo, OC]
        self.xt.fill(0x3C)
        w = r.uniform(-0.05, 0.05, (self.oc, self.c // self.g, self.k)).astype(np.float32)
        self.bias = DeviceBuffer.from_numpy(np.zeros(self.oc, np.float32))
        self.flops = 2.0 * n * self.lo * self.oc * (self.c // self.g) * self.k
        self.moved = (n * self.c * l + n * self.oc * self.lo) * es
        # conv1d
        self.d1 = hipops.conv1d_desc(n, self.c, l, self.oc, self.k, self.s, self.p, self.d, self.g)
        self.w1 = DeviceBuffer.from_numpy(hipops.conv1d_pack_weights(w, self.g, half))
        self.k1 = H.si_hip_conv1d_kernel_name(C.byref(self.d1), self.x.ptr, self.y.ptr, 1 if half else 0).decode()
        # conv2d on the [N, 1, L, C] image
        self.d2 = hipops.SiConv2dDesc(n, 1, l, self.c, self.c, 1, self.lo, self.oc, self.oc, 1, self.k, 1, self.s, 1, self.d, 0, self.p, self.g, 1, 0, 0,
                                      self.oc, 0, 0.0)
        w4 = np.ascontiguousarray(w.reshape(self.oc, self.c // self.g, 1, self.k))
        self.kind2 = 1
        if half:
            self.kind2 = H.si_hip_conv2d_f16_supported(C.byref(self.d2))
        if not half or self.kind2 == 3:
            packed = np.zeros(H.si_hip_conv2d_weight_elems(C.byref(self.d2)), np.float32)
            _chk(H.si_hip_conv2d_pack_weight_host(C.byref(self.d2), w4.ctypes.data_as(C.c_void_p), packed.ctypes.data_as(C.c_void_p)), "pack")
            self.w2 = DeviceBuffer.from_numpy(packed)
        elif self.kind2 == 1:
            packed = np.zeros(H.si_hip_conv2d_f16_weight_elems(C.byref(self.d2)), np.float16)
            _chk(H.si_hip_conv2d_f16_pack_weight_host(C.byref(self.d2), w4.ctypes.data_as(C.c_void_p), packed.ctypes.data_as(C.c_void_p)), "pack f16")
            self.w2 = DeviceBuffer.from_numpy(packed)
        else:
            self.w2 = None
        self.k2 = "conv2d (fp16 kind %d)" % self.kind2 if half else H.si_hip_conv2d_kernel_name(C.byref(self.d2), C.c_void_p(self.xt.ptr)).decode()
        # the two transposes
        self.pin = hipops.permute_desc((n, l, self.c), (self.c * l, 1, l), form="tile")
        self.pout = hipops.permute_desc((n, self.oc, self.lo), (self.lo * self.oc, 1, self.oc), form="tile")
        self.permute = H.si_hip_permute_f16 if half else H.si_hip_permute_f32

    def conv1d(self):
        fn = self.H.si_hip_conv1d_f16 if self.half else self.H.si_hip_conv1d_f32
        _chk(fn(C.byref(self.d1), self.x.ptr, self.w1.ptr, self.bias.ptr, self.y.ptr, None), "conv1d")

    def conv2d(self):
        H = self.H
        if not self.half:
            _chk(H.si_hip_conv2d_f32(C.byref(self.d2), self.xt.ptr, self.w2.ptr, self.bias.ptr, None, self.yt.ptr, None), "conv2d")
        elif self.kind2 == 3:
            _chk(H.si_hip_conv2d_depthwise_f16(C.byref(self.d2), self.xt.ptr, self.w2.ptr, self.bias.ptr, None, self.yt.ptr, None), "conv2d depthwise f16")
        else:
            _chk(H.si_hip_conv2d_f16(C.byref(self.d2), self.xt.ptr, self.w2.ptr, self.bias.ptr, None, self.yt.ptr, 0, None), "conv2d f16")

    def conv2d_permuted(self):
        _chk(self.permute(C.byref(self.pin), self.x.ptr, self.xt.ptr, None), "permute in")
        self.conv2d()
        _chk(self.permute(C.byref(self.pout), self.yt.ptr, self.y.ptr, None), "permute out")

    def copy(self):
        words = self.moved // 2 // 4        # the copy reads and writes each word: half the bytes moved, as 4-byte words
        width = 64
        while words % width:
            width //= 2
        _chk(self.H.si_hip_copy_channels_f32(self.x.ptr, words // width, width, width, self.y.ptr, width, None), "copy")


class Candidate:
    def __init__(self, tag, name, kernel, fn):
        self.tag, self.name, self.kernel, self.launch = tag, name, kernel, fn


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--seconds", type=float, default=0.1)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--length", type=int, default=500)
    args = ap.parse_args()
    T = Timer()
    print("HIP-event windows >= %.2f s, %d alternating repeats, batch %d, L = %d.  kernel library: %s" % (
        args.seconds, args.repeats, args.batch, args.length, os.path.basename(_native.LIB_HIP_PATH)))
    for half in (False, True):
        for shape in SHAPES:
            P = Problem(shape, args.batch, args.length, half)
            cands = [Candidate("a", "conv1d", P.k1, P.conv1d)]
            if P.w2 is not None:
                cands += [Candidate("b", "conv2d on [N,1,L,C]", P.k2, P.conv2d), Candidate("p", "permute + conv2d + permute", P.k2, P.conv2d_permuted)]
            if P.g > 1 and P.moved // 8 <= P.x.nbytes // 4 and P.moved // 8 <= P.y.nbytes // 4:
                cands.append(Candidate("c", "copy of the same bytes", "copy_channels_kernel", P.copy))
            for c in cands:
                T.window(c, 0.02)
            times = [[] for _ in cands]
            for _ in range(args.repeats):
                for c, t in zip(cands, times):
                    t.append(T.window(c, args.seconds))
            med = {c.tag: float(np.median(t)) for c, t in zip(cands, times)}
            print("%s  %s  [N %d, C %d, L %d] -> [OC %d, Lo %d]" % ("fp16" if half else "fp32", P.name, P.n, P.c, P.l, P.oc, P.lo))
            for c, t in zip(cands, times):
                m = med[c.tag]
                print("    %s %-28s [%-34s] median %.4f ms  spread %4.1f %%  %6.2f TFLOP/s  %5.2f TB/s moved" % (
                    c.tag, c.name, c.kernel, m, 100 * (max(t) - min(t)) / m, P.flops / m * 1e-9, P.moved / m * 1e-9))
            line = "    ratios:"
            for tag in "bpc":
                if tag in med:
                    line += "  a / %s = %.2f" % (tag, med["a"] / med[tag])
            print(line, flush=True)


if __name__ == "__main__":
    main()
