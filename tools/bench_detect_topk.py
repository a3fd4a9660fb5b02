"""tools/bench_detect_topk.py -- speed of si_hip_detect_topk_postprocess_f32 (include/si_topk.h) against two yardsticks on the SAME device tensors.

A YOLOv10-sized raw head: n = 32 images, rows = 8400, classes = 80, max_det = 300, SI_DETECT_CHANNELS ([n][84][8400]), scores
sigmoid(2 z - 5) of a seeded normal z, at the thresholds 0.25 (deployment) and 0.001 (validation).  One process; every side runs on the null
stream and is timed with torch.cuda events around windows of >= --seconds of back-to-back calls after a warm-up, --repeats alternating
repeats, medians:
    k   the entry, multi_label = 1 (ten launches)
    k1  the entry, multi_label = 0
    a   torch: scores.transpose(1, 2).flatten(1).topk(300), label and row from the index, the boxes gathered (no threshold, no un-letterbox)
    a1  torch: scores.amax(1), topk(300) over the rows
    b   si_hip_detect_postprocess_f32 with nms_threshold = 1 (one label per row: the yardstick of k1 alone)
The floor is one pass over the scores, n * rows * classes * 4 bytes at HBM's 8 TB/s.  k's picks are compared with a's on
the way where the threshold cuts nothing off the best 300.  Run on an otherwise idle card, under a time limit:
  timeout -k 10 300 python tools/bench_detect_topk.py > profiles/detect_topk_<sha>.txt
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

N, ROWS, CLASSES, MAX_DET = 32, 8400, 80, 300
HBM_BYTES_PER_MS = 8e12 / 1e3


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--seconds", type=float, default=0.3)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "no device: this tool measures on the GPU only"
    H = _native.hip()
    g = torch.Generator().manual_seed(0)
    pred = torch.empty((N, 4 + CLASSES, ROWS))
    pred[:, :4] = torch.rand((N, 4, ROWS), generator=g) * 600 + 20
    pred[:, 4:] = torch.sigmoid(2 * torch.randn((N, CLASSES, ROWS), generator=g) - 5)
    pred = pred.cuda()
    scores = pred[:, 4:]
    dets = torch.zeros((N, MAX_DET, 6), device="cuda")
    counts = torch.zeros((N,), dtype=torch.int32, device="cuda")
    src_rows = torch.zeros((N, MAX_DET), dtype=torch.int32, device="cuda")
    out = _native.SiDetectPostOut(dets.data_ptr(), counts.data_ptr(), src_rows.data_ptr(), None, None)
    floor = N * ROWS * CLASSES * 4 / HBM_BYTES_PER_MS
    print("windows >= %.2f s, %d alternating repeats, torch.cuda events.  torch %s.  kernel library: %s" % (
        args.seconds, args.repeats, torch.__version__, os.path.relpath(_native.LIB_HIP_PATH, ROOT)))
    print("n=%d rows=%d classes=%d max_det=%d channels   one-pass floor %.4f ms (%.1f MB of scores at 8 TB/s)" % (
        N, ROWS, CLASSES, MAX_DET, floor, N * ROWS * CLASSES * 4e-6))

    def torch_topk():
        v, i = scores.transpose(1, 2).flatten(1).topk(MAX_DET)
        row = i // CLASSES
        return v, i % CLASSES, row, pred[:, :4].gather(2, row[:, None, :].expand(-1, 4, -1))

    def torch_amax_topk():
        conf, label = scores.max(1)
        v, row = conf.topk(MAX_DET)
        return v, label.gather(1, row), row, pred[:, :4].gather(2, row[:, None, :].expand(-1, 4, -1))

    for thr in (0.25, 0.001):
        sides = []
        for tag, multi_label in (("k", 1), ("k1", 0)):
            d = hipops.detect_topk_desc(N, ROWS, CLASSES, 0, "channels", "cxcywh", thr, multi_label, MAX_DET)
            ws = torch.zeros((hipops.detect_topk_workspace_bytes(d),), dtype=torch.uint8, device="cuda")

            def ours(d=d, ws=ws):
                rc = H.si_hip_detect_topk_postprocess_f32(C.byref(d), pred.data_ptr(), None, C.byref(out), ws.data_ptr(), ws.numel(), None)
                assert rc == 0, rc
            sides.append((tag, "si_hip_detect_topk_postprocess_f32 multi_label=%d" % multi_label, ours))
        sides.insert(1, ("a", "torch flatten(1).topk", torch_topk))
        sides.append(("a1", "torch amax + topk", torch_amax_topk))
        dn = hipops.detect_desc(N, ROWS, CLASSES, False, 0, "channels", "cxcywh", thr, 1.0, False, MAX_DET)
        wn = torch.zeros((hipops.detect_workspace_bytes(dn),), dtype=torch.uint8, device="cuda")

        def nms_entry():
            rc = H.si_hip_detect_postprocess_f32(C.byref(dn), pred.data_ptr(), None, C.byref(out), wn.data_ptr(), wn.numel(), None)
            assert rc == 0, rc
        sides.append(("b", "si_hip_detect_postprocess_f32 nms_threshold=1", nms_entry))

        sides[0][2]()
        v, label, row, _ = torch_topk()
        torch.cuda.synchronize()
        kept = int(counts.min())
        same = "not compared (a has no threshold)"
        if bool((v > thr).all()):
            same = "conf %s, label %s" % (bool((dets[:, :, 4] == v).all()), bool((dets[:, :, 5] == label.float()).all()))
        print("threshold %g   kept per image %d .. %d   k against a: %s" % (thr, kept, int(counts.max()), same))
        for _ in range(2):   # warm-up
            for _, _, call in sides:
                window(call, 0.02)
        times = {tag: [] for tag, _, _ in sides}
        for _ in range(args.repeats):
            for tag, _, call in sides:
                times[tag].append(window(call, args.seconds))
        med = {tag: float(np.median(t)) for tag, t in times.items()}
        for tag, name, _ in sides:
            t = times[tag]
            print("    %-2s [%-48s] %s ms   median %.4f ms   spread %.1f %%   %.1f x floor" % (
                tag, name, " ".join("%.4f" % x for x in t), med[tag], 100 * (max(t) - min(t)) / med[tag], med[tag] / floor))
        print("    k / a = %.3f   k1 / a1 = %.3f   k1 / b = %.3f" % (med["k"] / med["a"], med["k1"] / med["a1"], med["k1"] / med["b"]), flush=True)


if __name__ == "__main__":
    main()
