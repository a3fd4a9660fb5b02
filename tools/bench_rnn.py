#!/usr/bin/env python3
"""tools/bench_rnn.py -- what one nn.LSTM / nn.GRU layer of CRNN size costs in the step form (include/si_rnn.h): T launches of the step
kernel behind one projection launch.

    python3 tools/bench_rnn.py [--fp16] [--cell lstm|gru] [--forwards 20]
        runs relu -> the layer -> relu in an Engine (T = 26, N = 32, I = 512, H = 256, bidirectional by default) `forwards` times; meant to
        be run under `rocprofv3 --kernel-trace --output-format csv -d DIR -- python3 tools/bench_rnn.py ...`
    python3 tools/bench_rnn.py --summarise DIR [--t 26 --hidden 256 --dirs 2 --cell lstm --fp16]
        reads the *kernel_trace.csv under DIR (no device needed) and prints, over the forwards after the first: time per step and per layer,
        the share of the layer spent between its kernels (the T kernel boundaries), and the W_hh bytes one step reads from L2
        (dirs * G * H * H elements) against the step's time.
"""
import argparse
import csv
import glob
import os
import statistics
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def run(a):
    import numpy as np
    from simpleinfer_amd import modelgen as mg
    from simpleinfer_amd.engine import Engine
    b = mg.PnnxBuilder(seed=1)
    x = b.relu(b.input((a.t, a.batch, a.input)))
    y = (b.lstm if a.cell == "lstm" else b.gru)(x, a.hidden, bidirectional=a.dirs == 2)
    b.output(b.relu(y))
    with tempfile.TemporaryDirectory() as td:
        pp, bp = os.path.join(td, "m.pnnx.param"), os.path.join(td, "m.pnnx.bin")
        b.save(pp, bp)
        e = Engine(fp16=1 if a.fp16 else 0)
        e.load_model(pp, bp)
        data = np.random.Generator(np.random.Philox(1)).random((a.t, a.batch, a.input), dtype=np.float32)
        e.input(e.input_names()[0], data)
        for _ in range(a.forwards):
            e.forward()
        out = e.extract(e.output_names()[0])
        layer = [L for L in e.profile() if L["type"] in ("nn.LSTM", "nn.GRU")][0]
    assert np.isfinite(out).all()
    print("ran %d forwards of %s T=%d N=%d I=%d H=%d D=%d %s: kernel %s" % (a.forwards, a.cell, a.t, a.batch, a.input, a.hidden, a.dirs,
                                                                         "fp16" if a.fp16 else "fp32", layer["kernel"]))


def summarise(a):
    rows = []
    for path in glob.glob(os.path.join(a.summarise, "**", "*kernel_trace.csv"), recursive=True):
        with open(path) as f:
            for r in csv.DictReader(f):
                rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]))
    rows.sort()
    steps = [i for i, r in enumerate(rows) if "rnn_step_kernel" in r[2]]
    assert steps and len(steps) % a.t == 0, "%d step launches, not a multiple of T = %d" % (len(steps), a.t)
    layers = [steps[i:i + a.t] for i in range(0, len(steps), a.t)][1:]          # the first forward carries the one-time setup
    us = lambda ns: ns / 1000.0
    step_us, first_us, proj_us, span_us, gap_us = [], [], [], [], []
    for grp in layers:
        assert grp == list(range(grp[0], grp[0] + a.t)), "the steps of a layer are not consecutive launches"
        proj = rows[grp[0] - 1]
        first_us.append(us(rows[grp[0]][1] - rows[grp[0]][0]))
        step_us += [us(rows[i][1] - rows[i][0]) for i in grp[1:]]
        proj_us.append(us(proj[1] - proj[0]))
        span_us.append(us(rows[grp[-1]][1] - proj[0]))
        gap_us.append(us(sum(rows[i][0] - rows[i - 1][1] for i in grp)))
    gates = 4 if a.cell == "lstm" else 3
    whh = a.dirs * gates * a.hidden * a.hidden * (2 if a.fp16 else 4)
    med = statistics.median
    step, span, gaps = med(step_us), med(span_us), med(gap_us)
    print("%s %s T=%d H=%d D=%d: %d layers measured" % (a.cell, "fp16" if a.fp16 else "fp32", a.t, a.hidden, a.dirs, len(layers)))
    print("  projection kernel (%s): %.2f us" % (rows[layers[0][0] - 1][2][:60], med(proj_us)))
    print("  step kernel: first step (no product) %.2f us; steps 2..T median %.2f us (min %.2f, max %.2f)" % (med(first_us), step, min(step_us), max(step_us)))
    print("  layer, projection start to last step end: %.2f us = projection %.2f + steps %.2f + %d kernel boundaries %.2f (%.1f %% of the layer, %.2f us each)"
          % (span, med(proj_us), span - med(proj_us) - gaps, a.t, gaps, 100.0 * gaps / span, gaps / a.t))
    print("  W_hh read per step: %d bytes (dirs * G * H * H elements) = %.0f GB/s over the step's %.2f us" % (whh, whh / step / 1e3, step))


if __name__ == "__main__":
    p = argparse.ArgumentParser()
    p.add_argument("--summarise")
    p.add_argument("--fp16", action="store_true")
    p.add_argument("--cell", default="lstm", choices=("lstm", "gru"))
    p.add_argument("--forwards", type=int, default=20)
    p.add_argument("--t", type=int, default=26)
    p.add_argument("--batch", type=int, default=32)
    p.add_argument("--input", type=int, default=512)
    p.add_argument("--hidden", type=int, default=256)
    p.add_argument("--dirs", type=int, default=2)
    args = p.parse_args()
    summarise(args) if args.summarise else run(args)
