"""tools/bench_nearest.py -- speed of the fused nearest-row search (include/si_nearest.h) against the two ways to the same answer without it.

One process; everything runs on the null stream on the SAME device tensors and is timed with torch.cuda events around windows of >= --seconds
of back-to-back calls after a warm-up, --repeats alternating repeats, medians:
    n  si_hip_nearest_f32 / _f16: idx (and dist) of the k nearest, the split over R as the plan chooses (its second launch included)
    c  si_hip_cdist_f32 / _f16 in mm mode into a device buffer, then torch.argmin(-1) (k = 1) or torch.topk(2, largest=False) (k = 2) on it
    t  torch.cdist(x1, x2, compute_mode="use_mm_for_euclid_dist") and the same reduction
The indices of n and c are compared on the way (they must be equal but for ties the half-rounded matrix of c creates under fp16).
Run on an otherwise idle card, under a time limit:
  timeout -k 10 600 python tools/bench_nearest.py > profiles/nearest_<sha>.txt
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
from bench_cdist import window  # noqa: E402  (beside this file)

# (name, B, P, R, M, k)
SHAPES = [("vq", 1, 8192, 1024, 64, 1), ("vq", 1, 8192, 8192, 64, 1), ("matcher", 2, 1024, 1024, 256, 2), ("small-P", 1, 256, 16384, 64, 1)]


def one(name, B, P, R, M, k, half, args):
    H = _native.hip()
    dt = torch.float16 if half else torch.float32
    g = torch.Generator().manual_seed(0)
    x1, x2 = torch.randn((B, P, M), generator=g).to(dt).cuda(), torch.randn((B, R, M), generator=g).to(dt).cuda()
    D = torch.empty((B, P, R), dtype=dt, device="cuda")
    idx = torch.empty((B, P, k), dtype=torch.int32, device="cuda")
    dist = torch.empty((B, P, k), dtype=torch.float32, device="cuda")
    dn = hipops.nearest_desc((B, P, M), (B, R, M), k)
    dc = hipops.cdist_desc((B, P, M), (B, R, M), 2.0, "use_mm_for_euclid_dist")
    nbytes = H.si_hip_nearest_workspace_bytes(C.byref(dn))
    ws = torch.empty((max(nbytes, 8),), dtype=torch.uint8, device="cuda")
    splits = nbytes // (B * P * k * 8) if nbytes else 1
    kernel = H.si_hip_nearest_kernel_name(C.byref(dn), C.c_void_p(x1.data_ptr()), C.c_void_p(x2.data_ptr()), None, int(half)).decode()
    near, cdist = (H.si_hip_nearest_f16, H.si_hip_cdist_f16) if half else (H.si_hip_nearest_f32, H.si_hip_cdist_f32)
    reduce_ = (lambda d: d.argmin(-1)) if k == 1 else (lambda d: d.topk(2, dim=-1, largest=False).indices)

    def fused():
        rc = near(C.byref(dn), x1.data_ptr(), x2.data_ptr(), idx.data_ptr(), dist.data_ptr(), None, ws.data_ptr(), nbytes, None)
        assert rc == 0, rc

    def composed():
        rc = cdist(C.byref(dc), x1.data_ptr(), x2.data_ptr(), D.data_ptr(), None)
        assert rc == 0, rc
        return reduce_(D)

    def theirs():
        return reduce_(torch.cdist(x1, x2, p=2.0, compute_mode="use_mm_for_euclid_dist"))

    fused()
    want = composed().reshape(B, P, k)
    torch.cuda.synchronize()
    differ = int((idx.long() != want).any(-1).sum())
    for _ in range(2):   # warm-up
        for call in (fused, composed, theirs):
            window(call, 0.02)
    times = {"n": [], "c": [], "t": []}
    for _ in range(args.repeats):
        for tag, call in (("n", fused), ("c", composed), ("t", theirs)):
            times[tag].append(window(call, args.seconds))
    med = {tag: float(np.median(v)) for tag, v in times.items()}
    flop = 2.0 * B * P * R * M
    print("%s %s  B=%d P=%d R=%d M=%d k=%d   matrix %.1f MB   rows whose indices differ from c: %d of %d" % (
        name, "fp16" if half else "fp32", B, P, R, M, k, B * P * R * (2 if half else 4) / 1e6, differ, B * P))
    names = {"n": "%s, splits=%d" % (kernel, splits), "c": "si_hip_cdist + torch reduction", "t": "torch %s cdist + reduction" % torch.__version__}
    for tag in ("n", "c", "t"):
        t = times[tag]
        print("    %s [%-48s] %s ms   median %.4f ms   %.1f TFLOP/s   spread %.1f %%" % (tag, names[tag], " ".join("%.4f" % v for v in t), med[tag],
                                                                                       flop / med[tag] * 1e-9, 100 * (max(t) - min(t)) / med[tag]))
    print("    n / c = %.3f   n / t = %.3f" % (med["n"] / med["c"], med["n"] / med["t"]), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--seconds", type=float, default=0.3)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "no device: this tool measures on the GPU only"
    print("windows >= %.2f s, %d alternating repeats, torch.cuda events.  kernel library: %s" % (args.seconds, args.repeats, os.path.relpath(_native.LIB_HIP_PATH, ROOT)))
    for shape in SHAPES:
        for half in (False, True):
            one(*shape, half, args)


if __name__ == "__main__":
    main()
