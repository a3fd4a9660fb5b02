"""examples/yolov8_seg_demo.py -- an anchor-free segmentation head end to end on the device, modelled on examples/yolo_demo.py:
letterbox packing -> Engine::Forward -> detect_postprocess (filter / sort / NMS / un-letterbox, the mask coefficients carried along) ->
detect_masks (coefficients x prototypes, cropped to the box), with synthetic "photos" and a toy network with seeded random weights
(modelgen.build_toy_yolov8_seg: the boxes mean nothing, and the threshold is set where its scores leave a few per cent of the rows -- the
point is the data flow).  Both graph outputs stay in HBM (outputs_to_host=0): the channel-major head [N, 4 + nc + nm, cells] is read where
the engine left it, without a permute, and so are the prototypes; only dets, counts and the mask planes of the kept detections are copied
to the host.

    python examples/yolov8_seg_demo.py [--size 256] [--images 4] [--rows]
"""
import argparse
import os
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import simpleinfer_amd as si  # noqa: E402
from simpleinfer_amd import hipops  # noqa: E402


def run(size=256, images=((480, 640), (1080, 810), (375, 500), (720, 1280)), nc=5, nm=32, channels_first=True, prob_threshold=0.45, max_det=100, seed=0):
    mg = si.modelgen
    n = len(images)
    rng = np.random.Generator(np.random.Philox(seed))
    with tempfile.TemporaryDirectory() as td:
        pp, bp = os.path.join(td, "m.pnnx.param"), os.path.join(td, "m.pnnx.bin")
        mg.build_toy_yolov8_seg(n, size, nc, nm, channels_first).save(pp, bp)
        e = si.Engine(outputs_to_host=0)
        e.load_model(pp, bp)
        x = np.empty((n, size, size, 3), np.float32)
        adjust = np.empty((n, 5), np.float32)
        for b, (h, w) in enumerate(images):
            hr, wr, scale, pt, pl = hipops.letterbox_geometry(h, w, size, size)
            resized = rng.integers(0, 256, (hr, wr, 3), dtype=np.uint8)   # stands in for cv::resize(imread(...))
            x[b] = hipops.letterbox(resized, size, size, pt, pl)           # pad / BGR->RGB / float / /255 on the device
            adjust[b] = (pl, pt, scale, w, h)
        e.input("0", x)
        e.forward()
        head_name, proto_name = e.output_names()
        (hptr, _), (pptr, _) = e.extract_ptr(head_name), e.extract_ptr(proto_name)
        head_shape, proto_shape = e.operand_shape(head_name), e.operand_shape(proto_name)     # [N, no, cells] | [N, cells, no]; NHWC [N, mh, mw, nm]
        no = 4 + nc + nm
        cells = head_shape[2] if channels_first else head_shape[1]
        head = hipops.DeviceBuffer.view(hptr, n * no * cells * 4)
        res = hipops.detect_postprocess(None, nc, objectness=False, extra=nm, layout="channels" if channels_first else "rows", prob_threshold=prob_threshold,
                                        nms_threshold=0.45, adjust=adjust, max_det=max_det, pred_dev=head, shape=(n, cells), host=("dets", "counts"), stream=e.stream())
        mh, mw = proto_shape[1], proto_shape[2]
        protos = hipops.DeviceBuffer.view(pptr, int(np.prod(proto_shape)) * 4)
        masks = hipops.detect_masks(None, res, None, None, np.float32(mw) / np.float32(size), np.float32(mh) / np.float32(size), protos_dev=protos,
                                    shape=proto_shape, stream=e.stream())
    return res, masks, cells


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--images", type=int, default=4)
    ap.add_argument("--rows", action="store_true", help="the export with the closing permute: [N, cells, no]")
    a = ap.parse_args()
    shapes = ((480, 640), (1080, 810), (375, 500), (720, 1280))[:a.images]
    res, masks, cells = run(a.size, shapes, channels_first=not a.rows)
    for b, d in enumerate(res.dets):
        print("image %d (%dx%d): %d boxes kept of %d predictions (%d stored); mask pixels per box: %s; first: %s" % (
            b, shapes[b][1], shapes[b][0], res.counts[b], cells, len(d), [int(m.sum()) for m in masks[b]][:8],
            np.array2string(d[0], precision=2) if len(d) else "-"))
