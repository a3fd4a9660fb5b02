"""examples/yolov10_demo.py -- an end-to-end (NMS-free) head on the device, in the shape of examples/yolov8_obb_demo.py: letterbox packing ->
Engine::Forward -> detect_topk_postprocess (the max_det best (row, class) pairs by a radix select, label and row from the flat index, the
un-letterbox of the boxes), with synthetic "photos" and a toy network with seeded random weights (modelgen.build_toy_yolov10_head; the boxes
mean nothing -- the point is the data flow).  The top-k of such a head cannot stand in the graph, so the head is exported raw: [N, 4 + nc,
cells] stays in HBM (outputs_to_host=0) and is read where the engine left it; only the kept rows [k][6] and the counts are copied to the host.
One row may come out with several labels.

    python examples/yolov10_demo.py [--size 256] [--images 4] [--rows] [--single-label]
"""
import argparse
import os
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import simpleinfer_amd as si  # noqa: E402
from simpleinfer_amd import hipops  # noqa: E402


def run(size=256, images=((480, 640), (1080, 810), (375, 500), (720, 1280)), nc=5, channels_first=True, prob_threshold=0.25, max_det=300,
        multi_label=True, seed=0):
    n = len(images)
    rng = np.random.Generator(np.random.Philox(seed))
    with tempfile.TemporaryDirectory() as td:
        pp, bp = os.path.join(td, "m.pnnx.param"), os.path.join(td, "m.pnnx.bin")
        si.modelgen.build_toy_yolov10_head(n, size, nc, channels_first).save(pp, bp)
        e = si.Engine(outputs_to_host=0)
        e.load_model(pp, bp)
        x = np.empty((n, size, size, 3), np.float32)
        adjust = np.empty((n, 5), np.float32)
        for b, (h, w) in enumerate(images):
            hr, wr, scale, pt, pl = hipops.letterbox_geometry(h, w, size, size)
            resized = rng.integers(0, 256, (hr, wr, 3), dtype=np.uint8)   # stands in for cv::resize(imread(...))
            x[b] = hipops.letterbox(resized, size, size, pt, pl)
            adjust[b] = (pl, pt, scale, w, h)
        e.input("0", x)
        e.forward()
        head_name = e.output_names()[0]
        hptr, _ = e.extract_ptr(head_name)
        head_shape = e.operand_shape(head_name)                            # [N, no, cells] | [N, cells, no]
        cells = head_shape[2] if channels_first else head_shape[1]
        head = hipops.DeviceBuffer.view(hptr, n * (4 + nc) * cells * 4)
        res = hipops.detect_topk_postprocess(None, nc, layout="channels" if channels_first else "rows", prob_threshold=prob_threshold,
                                             multi_label=multi_label, adjust=adjust, max_det=max_det, pred_dev=head, shape=(n, cells),
                                             want=("src_rows",), stream=e.stream())
    return res, cells


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--images", type=int, default=4)
    ap.add_argument("--rows", action="store_true", help="the export with the closing permute: [N, cells, no]")
    ap.add_argument("--single-label", action="store_true", help="one candidate per row: its first-maximum class")
    a = ap.parse_args()
    shapes = ((480, 640), (1080, 810), (375, 500), (720, 1280))[:a.images]
    res, cells = run(a.size, shapes, channels_first=not a.rows, multi_label=not a.single_label)
    for b, d in enumerate(res.dets):
        print("image %d (%dx%d): %d candidates above the threshold of %d predictions, %d stored (%d distinct rows); best: %s" % (
            b, shapes[b][1], shapes[b][0], res.counts[b], cells, len(d), len(set(res.src_rows[b])), np.array2string(d[0], precision=2) if len(d) else "-"))
