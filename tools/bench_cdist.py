"""tools/bench_cdist.py -- speed of cdist_mm_kernel (include/si_cdist.h) against the installed torch's torch.cdist on the SAME device tensors.

The matcher's shape: B = 2, P = R = 1024, M = 256, p = 2, fp32 and fp16.  One process; both sides run on the null stream and are timed with
torch.cuda events around windows of >= --seconds of back-to-back calls after a warm-up, --repeats alternating repeats, medians:
    c  si_hip_cdist_f32 / _f16 on the torch tensors' own pointers, into a torch tensor
    t  torch.cdist(x1, x2, compute_mode="use_mm_for_euclid_dist") (its own output allocation, from torch's caching allocator)
FLOP / s counts 2 B P R M, the product alone.  The two results are compared on the way (max |c - t| over max |t|).
Run on an otherwise idle card, under a time limit:
  timeout -k 10 300 python tools/bench_cdist.py > profiles/cdist_<sha>.txt
"""
import argparse
import ctypes as C
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from simpleinfer_amd import _native, hipops  # noqa: E402

B, P, R, M = 2, 1024, 1024, 256


def window(call, seconds):
    """mean ms per call over a window of >= seconds"""
    def timed(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            call()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)
    est = timed(10) / 10
    iters = max(20, int(seconds * 1000.0 / max(est, 1e-3)) + 1)
    return timed(iters) / iters


def one(half, args):
    H = _native.hip()
    dt = torch.float16 if half else torch.float32
    g = torch.Generator().manual_seed(0)
    x1, x2 = torch.randn((B, P, M), generator=g).to(dt).cuda(), torch.randn((B, R, M), generator=g).to(dt).cuda()
    out = torch.empty((B, P, R), dtype=dt, device="cuda")
    d = hipops.cdist_desc((B, P, M), (B, R, M), 2.0, "use_mm_for_euclid_dist")
    kernel = H.si_hip_cdist_kernel_name(C.byref(d), C.c_void_p(x1.data_ptr()), C.c_void_p(x2.data_ptr()), C.c_void_p(out.data_ptr()), int(half)).decode()
    fn = H.si_hip_cdist_f16 if half else H.si_hip_cdist_f32

    def ours():
        rc = fn(C.byref(d), x1.data_ptr(), x2.data_ptr(), out.data_ptr(), None)
        assert rc == 0, rc

    def theirs():
        return torch.cdist(x1, x2, p=2.0, compute_mode="use_mm_for_euclid_dist")

    ours()
    ref = theirs()
    torch.cuda.synchronize()
    diff = float((out.double() - ref.double()).abs().max() / ref.double().abs().max())
    for _ in range(2):   # warm-up
        window(ours, 0.02)
        window(theirs, 0.02)
    tc, tt = [], []
    for _ in range(args.repeats):
        tc.append(window(ours, args.seconds))
        tt.append(window(theirs, args.seconds))
    mc, mt = float(np.median(tc)), float(np.median(tt))
    flop = 2.0 * B * P * R * M
    print("%s  B=%d P=%d R=%d M=%d   max|c - t| / max|t| = %.2e" % ("fp16" if half else "fp32", B, P, R, M, diff))
    for tag, name, t, m in (("c", kernel, tc, mc), ("t", "torch %s torch.cdist" % torch.__version__, tt, mt)):
        print("    %s [%-36s] %s ms   median %.4f ms   %.1f TFLOP/s   spread %.1f %%" % (tag, name, " ".join("%.4f" % v for v in t), m, flop / m * 1e-9,
                                                                                       100 * (max(t) - min(t)) / m))
    print("    c / t = %.3f" % (mc / mt), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--seconds", type=float, default=0.3)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "no device: this tool measures on the GPU only"
    print("windows >= %.2f s, %d alternating repeats, torch.cuda events.  kernel library: %s" % (args.seconds, args.repeats, os.path.relpath(_native.LIB_HIP_PATH, ROOT)))
    for half in (False, True):
        one(half, args)


if __name__ == "__main__":
    main()
