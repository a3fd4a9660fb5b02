"""examples/yolov8_obb_demo.py -- an anchor-free oriented-box head end to end on the device, in the shape of examples/yolov8_seg_demo.py:
letterbox packing -> Engine::Forward -> detect_obb_postprocess (filter / sort / rotated NMS by ProbIoU / un-letterbox of centre and size, the
angle carried along), with synthetic "photos" and a toy network with seeded random weights (modelgen.build_toy_yolov8_seg, whose payload
channels stand in for an `-obb` head's: payload element 0 is read as the angle in radians; the boxes mean nothing -- the point is the data
flow).  The head [N, 4 + nc + extra, cells] stays in HBM (outputs_to_host=0) and is read where the engine left it, without a permute; only
the kept rows [k][7] = cx, cy, w, h, angle, confidence, label and the counts are copied to the host.

    python examples/yolov8_obb_demo.py [--size 256] [--images 4] [--rows]
"""
import argparse
import os
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import simpleinfer_amd as si  # noqa: E402
from simpleinfer_amd import hipops  # noqa: E402


def run(size=256, images=((480, 640), (1080, 810), (375, 500), (720, 1280)), nc=5, extra=32, channels_first=True, prob_threshold=0.45, max_det=100, seed=0):
    mg = si.modelgen
    n = len(images)
    rng = np.random.Generator(np.random.Philox(seed))
    with tempfile.TemporaryDirectory() as td:
        pp, bp = os.path.join(td, "m.pnnx.param"), os.path.join(td, "m.pnnx.bin")
        mg.build_toy_yolov8_seg(n, size, nc, extra, channels_first).save(pp, bp)
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
        no = 4 + nc + extra
        cells = head_shape[2] if channels_first else head_shape[1]
        head = hipops.DeviceBuffer.view(hptr, n * no * cells * 4)
        res = hipops.detect_obb_postprocess(None, nc, extra=extra, angle_off=0, layout="channels" if channels_first else "rows",
                                            prob_threshold=prob_threshold, nms_threshold=0.45, adjust=adjust, max_det=max_det, pred_dev=head,
                                            shape=(n, cells), want=("src_rows",), stream=e.stream())
    return res, cells


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--images", type=int, default=4)
    ap.add_argument("--rows", action="store_true", help="the export with the closing permute: [N, cells, no]")
    a = ap.parse_args()
    shapes = ((480, 640), (1080, 810), (375, 500), (720, 1280))[:a.images]
    res, cells = run(a.size, shapes, channels_first=not a.rows)
    for b, d in enumerate(res.obbs):
        print("image %d (%dx%d): %d oriented boxes kept of %d predictions (%d stored); first: %s" % (
            b, shapes[b][1], shapes[b][0], res.counts[b], cells, len(d), np.array2string(d[0], precision=2) if len(d) else "-"))
