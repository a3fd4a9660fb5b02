"""tools/bench_attention.py -- speed of si_hip_attention_f32 / _f16 (include/si_attention.h) against two yardsticks on the same card in
the same run.

Shapes: the C3TR block of YOLOv5s-transformer at 640 (L = 400 tokens, E = 256, 4 heads of 64; batch 1 and 32) and an MHSA shape (L = 196,
E = 384, 6 heads of 64; batch 1 and 32), fp32 and fp16.  Q | K | V are the column slices of one [rows, 3E] buffer, as the layer's workspace
is.  Per shape, each candidate timed in one process in alternating windows:
  a  the fused kernel, one launch
  t  torch.nn.functional.scaled_dot_product_attention of the installed torch on the same values ([N, heads, L, d] tensors)
  u  the unfused composition through this project's own entries, per (batch item, head): the 1x1-conv GEMM S = Q K^T (K packed as the
     weights, the scale folded in), si_hip_softmax over the rows of S, the 1x1-conv GEMM P V -- three launches and the L x L matrix
     written and read twice.  (fp16: needs L % 8 == 0, so the MHSA shape has no u row.)
Windows of >= --seconds, --repeats alternating repeats; prints the medians, achieved FLOP/s (4 N heads L L d, counted from shapes) against
the fp32 MFMA rate 157.3 TF/s, and the ratios t / a and u / a.  Run on an otherwise idle card under a time limit:
  timeout -k 10 600 python tools/bench_attention.py > profiles/attention_<sha>.txt
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

PEAK_F32_MFMA = 157.3e12


def data(batch, length, e, half, seed):
    r = np.random.Generator(np.random.Philox(seed))
    return (r.random((batch, length, e), dtype=np.float32) * 2 - 1).astype(np.float16 if half else np.float32)


class Fused:
    tag = "a"

    def __init__(self, batch, length, heads, d, half, q, k, v):
        self.H = H = _native.hip()
        e = heads * d
        es = 2 if half else 4
        self.d = hipops.attention_desc(batch, heads, length, length, d, batch_first=True, q_ld=3 * e, k_ld=3 * e, v_ld=3 * e)
        self.ws = DeviceBuffer.from_numpy(np.concatenate([q, k, v], axis=2))
        self.out = DeviceBuffer(batch * length * e * es)
        self.ptr = [self.ws.ptr + j * e * es for j in range(3)]
        self.fn = H.si_hip_attention_f16 if half else H.si_hip_attention_f32
        self.kernel = H.si_hip_attention_kernel_name(C.byref(self.d), self.ptr[0], self.ptr[1], self.ptr[2], self.out.ptr, 1 if half else 0).decode()

    def launch(self):
        _chk(self.fn(C.byref(self.d), self.ptr[0], self.ptr[1], self.ptr[2], self.out.ptr, None), "attention")


class Torch:
    tag = "t"

    def __init__(self, batch, length, heads, d, half, q, k, v):
        import torch
        self.F = torch.nn.functional
        split = lambda t: torch.from_numpy(np.ascontiguousarray(t.reshape(batch, length, heads, d).transpose(0, 2, 1, 3))).cuda()
        self.q, self.k, self.v = split(q), split(k), split(v)
        self.kernel = "torch %s sdpa" % torch.__version__

    def launch(self):
        self.o = self.F.scaled_dot_product_attention(self.q, self.k, self.v)


class Unfused:
    tag = "u"

    def __init__(self, batch, length, heads, d, half, q, k, v):
        self.H = H = _native.hip()
        self.half = half
        es = 2 if half else 4
        e = heads * d
        scale = 1.0 / np.sqrt(d)
        L = length
        desc = lambda ic, in_ld, oc, out_ld: hipops.SiConv2dDesc(L, 1, 1, ic, in_ld, 1, 1, oc, out_ld, 1, 1, 1, 1, 1, 1, 0, 0, 1, 0, 0, 0, oc, 0, 0.0)
        self.d_s, self.d_o = desc(d, e, L, L), desc(L, L, d, e)
        self.d_sm = hipops.softmax_desc((L, 1, 1, L), 3)
        self.q = DeviceBuffer.from_numpy(q)
        self.s, self.p = DeviceBuffer(L * L * es), DeviceBuffer(L * L * es)
        self.out = DeviceBuffer(batch * L * e * es)
        elems, pack = ((H.si_hip_conv2d_f16_weight_elems, H.si_hip_conv2d_f16_pack_weight_host) if half else
                       (H.si_hip_conv2d_weight_elems, H.si_hip_conv2d_pack_weight_host))

        def packed(dsc, w_oi):
            w = np.ascontiguousarray(w_oi.astype(np.float32))
            img = np.zeros(elems(C.byref(dsc)), np.float16 if half else np.float32)
            _chk(pack(C.byref(dsc), w.ctypes.data_as(C.c_void_p), img.ctypes.data_as(C.c_void_p)), "pack")
            return DeviceBuffer.from_numpy(img)

        self.items = []
        for b in range(batch):
            for h in range(heads):
                sl = slice(h * d, (h + 1) * d)
                wk = packed(self.d_s, k[b][:, sl].astype(np.float32) * scale)          # [oc = keys, ic = d]
                wv = packed(self.d_o, v[b][:, sl].astype(np.float32).T)                # [oc = d, ic = keys]
                off = (b * L * e + h * d) * es
                self.items.append((self.q.ptr + off, wk, wv, self.out.ptr + off))
        self.kernel = "conv 1x1 -> softmax -> conv 1x1, %d launches" % (3 * len(self.items))

    def launch(self):
        H = self.H
        for qp, wk, wv, op in self.items:
            if self.half:
                _chk(H.si_hip_conv2d_f16(C.byref(self.d_s), qp, wk.ptr, None, None, self.s.ptr, 0, None), "S")
                _chk(H.si_hip_softmax_f16(C.byref(self.d_sm), self.s.ptr, self.p.ptr, None), "softmax")
                _chk(H.si_hip_conv2d_f16(C.byref(self.d_o), self.p.ptr, wv.ptr, None, None, op, 0, None), "PV")
            else:
                _chk(H.si_hip_conv2d_f32(C.byref(self.d_s), qp, wk.ptr, None, None, self.s.ptr, None), "S")
                _chk(H.si_hip_softmax_f32(C.byref(self.d_sm), self.s.ptr, self.p.ptr, None), "softmax")
                _chk(H.si_hip_conv2d_f32(C.byref(self.d_o), self.p.ptr, wv.ptr, None, None, op, None), "PV")


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
        est = self.time(case, 3) / 3
        iters = max(5, int(seconds * 1000.0 / max(est, 1e-3)) + 1)
        ms = self.time(case, iters)
        while ms < seconds * 1000.0:
            iters = int(iters * seconds * 1000.0 / max(ms, 1e-3) * 1.1) + 1
            ms = self.time(case, iters)
        return ms / iters


def compare(T, name, flops, cases, args):
    for c in cases:   # warm-up
        T.window(c, 0.02)
    times = [[] for _ in cases]
    for _ in range(args.repeats):
        for c, t in zip(cases, times):
            t.append(T.window(c, args.seconds))
    med = [float(np.median(t)) for t in times]
    print(name)
    for c, t, m in zip(cases, times, med):
        print("    %s [%-46s] median %8.4f ms  %6.2f TF/s = %4.1f %% of %.1f  spread %4.1f %%  / a = %.2f" % (
            c.tag, c.kernel, m, flops / m * 1e-9, 100 * flops / m * 1e3 / PEAK_F32_MFMA, PEAK_F32_MFMA * 1e-12, 100 * (max(t) - min(t)) / m, m / med[0]))
    sys.stdout.flush()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--seconds", type=float, default=0.1)
    ap.add_argument("--no-torch", action="store_true")
    args = ap.parse_args()
    T = Timer()
    print("HIP-event windows >= %.2f s, %d alternating repeats.  kernel library: %s" % (args.seconds, args.repeats, os.path.basename(_native.LIB_HIP_PATH)))
    for half in (False, True):
        for what, length, heads, d, batches in (("C3TR 640", 400, 4, 64, (1, 32)), ("MHSA", 196, 6, 64, (1, 32))):
            for batch in batches:
                e = heads * d
                q, k, v = (data(batch, length, e, half, s) for s in (1, 2, 3))
                kinds = [Fused] + ([] if args.no_torch else [Torch]) + ([Unfused] if not half or length % 8 == 0 else [])
                cases = [K(batch, length, heads, d, half, q, k, v) for K in kinds]
                compare(T, "%s  L = %d, E = %d, %d heads, batch %d, %s" % (what, length, e, heads, batch, "fp16" if half else "fp32"),
                        4.0 * batch * heads * length * length * d, cases, args)


if __name__ == "__main__":
    main()
