"""tools/bench_xcorr.py -- speed of the cross-correlation kernels (include/si_xcorr.h) against the code the project had before them.

The yardstick is nn.Conv2d's own launch with the same values as CONSTANT weights on the same shapes -- which is what a graph could run only if
the filter never changed.  It is reported twice: the launch alone (b), and the launch behind the host pack of its weight image and the upload
(u), which a tensor filter would pay on every forward (on top of bringing the filter to the host, which is not counted).  Shapes, fp32 and
fp16 storage:
  SiamFC      256 ch, 22x22 * 6x6, O = 1
  SiamRPN     256 ch, 20x20 * 4x4, 2k = 10 filters
  SiamRPN++   depthwise 256 ch, 31x31 * 7x7, N = 1 and 8 (a: ONE per-sample launch on [N, H, W, C]; b: the conv on the folded [1, H, W, N C])
  SOLO        256 -> 128 1x1 on 200x304
a and b are timed in one process in alternating HIP-event windows of >= --seconds, --repeats times, and the median is printed with the spread
of the windows; u is wall-clock time per forward over --pack-iters forwards.  Ratios below 1: the new kernel is faster.
Run on an otherwise idle card under a time limit:
  timeout -k 10 600 python tools/bench_xcorr.py > profiles/xcorr_<sha>.txt
"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from simpleinfer_amd import _native, hipops  # noqa: E402
from simpleinfer_amd.hipops import DeviceBuffer, _chk  # noqa: E402
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_layout import Timer  # noqa: E402

# (name, N, C, H, W, O, kh, kw, depthwise)
SHAPES = [("SiamFC 256ch 22x22 * 6x6, O 1", 1, 256, 22, 22, 1, 6, 6, False), ("SiamRPN 256ch 20x20 * 4x4, O 10", 1, 256, 20, 20, 10, 4, 4, False),
          ("SiamRPN++ depthwise 256ch 31x31 * 7x7, N 1", 1, 256, 31, 31, 256, 7, 7, True),
          ("SiamRPN++ depthwise 256ch 31x31 * 7x7, N 8", 8, 256, 31, 31, 256, 7, 7, True), ("SOLO 256 -> 128 1x1 on 200x304", 1, 256, 200, 304, 128, 1, 1, False)]


class Problem:
    """one shape in one storage type: the buffers every candidate shares"""

    def __init__(self, shape, half):
        self.H = H = _native.hip()
        self.name, self.n, self.c, self.h, self.w, self.oc, self.kh, self.kw, self.dw = shape
        self.half = half
        n, c, h, w, oc, kh, kw = self.n, self.c, self.h, self.w, self.oc, self.kh, self.kw
        self.ho, self.wo = h - kh + 1, w - kw + 1
        dt = np.float16 if half else np.float32
        es = 2 if half else 4
        r = np.random.Generator(np.random.Philox(1))
        self.x = DeviceBuffer.from_numpy(r.uniform(-1, 1, (n, h, w, c)).astype(dt))
        self.y = DeviceBuffer(n * self.ho * self.wo * oc * es)
        self.bias = DeviceBuffer.from_numpy(np.zeros(n * oc, np.float32))
        if self.dw:
            z = r.uniform(-0.1, 0.1, (n, c, kh, kw)).astype(np.float32)                 # the templates, torch's layout
            self.wt = DeviceBuffer.from_numpy(np.ascontiguousarray(z.transpose(0, 2, 3, 1)).astype(dt))      # [N][kh][kw][C] as stored
            self.d1 = hipops.xcorr_desc(n, h, w, c, c, kh, kw, groups=c, per_sample=True)
            w4 = np.ascontiguousarray(z.reshape(n * c, 1, kh, kw))
            fold, g = n * c, n * c
            self.flops = 2.0 * n * self.ho * self.wo * c * kh * kw
        else:
            wf = r.uniform(-0.05, 0.05, (oc, c, kh, kw)).astype(np.float32)
            self.wt = DeviceBuffer.from_numpy(np.ascontiguousarray(wf.transpose(0, 2, 3, 1)).astype(dt))     # [O][kh][kw][C] as stored
            self.d1 = hipops.xcorr_desc(n, h, w, c, oc, kh, kw)
            w4, fold, g = wf, c, 1
            self.flops = 2.0 * n * self.ho * self.wo * oc * c * kh * kw
        self.k1 = H.si_hip_xcorr_kernel_name(C.byref(self.d1), self.x.ptr, self.wt.ptr, self.y.ptr, 1 if half else 0).decode()
        # nn.Conv2d's launch: the depthwise problem folded to [1, H, W, N C] with N C filters, as the unfused sandwich runs it
        on, ooc = (1, fold) if self.dw else (n, oc)
        self.w4 = w4
        self.d2 = hipops.SiConv2dDesc(on, h, w, fold, fold, self.ho, self.wo, ooc, ooc, kh, kw, 1, 1, 1, 1, 0, 0, g, 1, 0, 0, ooc, 0, 0.0)
        self.kind2 = H.si_hip_conv2d_f16_supported(C.byref(self.d2)) if half else 1
        self.w2 = None
        if not half or self.kind2 in (1, 3):
            self.w2 = DeviceBuffer.from_numpy(self.pack())
        self.k2 = ("conv2d (fp16 kind %d)" % self.kind2) if half else H.si_hip_conv2d_kernel_name(C.byref(self.d2), C.c_void_p(self.x.ptr)).decode()

    def pack(self):
        H = self.H
        if not self.half or self.kind2 == 3:
            packed = np.zeros(H.si_hip_conv2d_weight_elems(C.byref(self.d2)), np.float32)
            _chk(H.si_hip_conv2d_pack_weight_host(C.byref(self.d2), self.w4.ctypes.data_as(C.c_void_p), packed.ctypes.data_as(C.c_void_p)), "pack")
        else:
            packed = np.zeros(H.si_hip_conv2d_f16_weight_elems(C.byref(self.d2)), np.float16)
            _chk(H.si_hip_conv2d_f16_pack_weight_host(C.byref(self.d2), self.w4.ctypes.data_as(C.c_void_p), packed.ctypes.data_as(C.c_void_p)), "pack f16")
        return packed

    def xcorr(self):
        fn = self.H.si_hip_xcorr_f16 if self.half else self.H.si_hip_xcorr_f32
        _chk(fn(C.byref(self.d1), self.x.ptr, self.wt.ptr, self.bias.ptr, self.y.ptr, None), "xcorr")

    def conv2d(self):
        H = self.H
        if not self.half:
            _chk(H.si_hip_conv2d_f32(C.byref(self.d2), self.x.ptr, self.w2.ptr, self.bias.ptr, None, self.y.ptr, None), "conv2d")
        elif self.kind2 == 3:
            _chk(H.si_hip_conv2d_depthwise_f16(C.byref(self.d2), self.x.ptr, self.w2.ptr, self.bias.ptr, None, self.y.ptr, None), "conv2d depthwise f16")
        else:
            _chk(H.si_hip_conv2d_f16(C.byref(self.d2), self.x.ptr, self.w2.ptr, self.bias.ptr, None, self.y.ptr, 0, None), "conv2d f16")

    def conv2d_packed_each_forward(self, iters):
        """wall-clock ms per forward: host pack of the weight image, upload into the existing buffer, launch; one sync at the end"""
        H = self.H
        _chk(H.si_hip_stream_sync(None), "sync")
        t0 = time.perf_counter()
        for _ in range(iters):
            packed = self.pack()
            _chk(H.si_hip_memcpy_h2d(self.w2.ptr, packed.ctypes.data_as(C.c_void_p), packed.nbytes, None), "h2d")
            self.conv2d()
        _chk(H.si_hip_stream_sync(None), "sync")
        return (time.perf_counter() - t0) * 1e3 / iters


class Candidate:
    def __init__(self, tag, name, kernel, fn):
        self.tag, self.name, self.kernel, self.launch = tag, name, kernel, fn


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--seconds", type=float, default=0.1)
    ap.add_argument("--pack-iters", type=int, default=20)
    args = ap.parse_args()
    T = Timer()
    print("HIP-event windows >= %.2f s, %d alternating repeats; pack + upload: wall clock over %d forwards.  kernel library: %s" % (
        args.seconds, args.repeats, args.pack_iters, os.path.basename(_native.LIB_HIP_PATH)))
    for half in (False, True):
        for shape in SHAPES:
            P = Problem(shape, half)
            cands = [Candidate("a", "xcorr, the filter a tensor", P.k1, P.xcorr)]
            if P.w2 is not None:
                cands.append(Candidate("b", "conv2d, constant weights", P.k2, P.conv2d))
            for c in cands:
                T.window(c, 0.02)
            times = [[] for _ in cands]
            for _ in range(args.repeats):
                for c, t in zip(cands, times):
                    t.append(T.window(c, args.seconds))
            med = {c.tag: float(np.median(t)) for c, t in zip(cands, times)}
            print("%s  %s  [N %d, %dx%d, C %d] * [%dx%d] -> [%dx%d, O %d]" % ("fp16" if half else "fp32", P.name, P.n, P.h, P.w, P.c, P.kh, P.kw, P.ho, P.wo, P.oc))
            for c, t in zip(cands, times):
                m = med[c.tag]
                print("    %s %-28s [%-34s] median %.4f ms  spread %4.1f %%  %7.3f TFLOP/s" % (
                    c.tag, c.name, c.kernel, m, 100 * (max(t) - min(t)) / m, P.flops / m * 1e-9))
            line = "    ratios:"
            if "b" in med:
                P.conv2d_packed_each_forward(3)
                u = P.conv2d_packed_each_forward(args.pack_iters)
                print("    u %-28s [%-34s] %.4f ms per forward (wall clock)" % ("conv2d + host pack + upload", P.k2, u))
                line += "  a / b = %.2f  a / u = %.3f" % (med["a"] / med["b"], med["a"] / u)
            else:
                line += "  (the fp16 conv2d does not serve this shape)"
            print(line, flush=True)


if __name__ == "__main__":
    main()
