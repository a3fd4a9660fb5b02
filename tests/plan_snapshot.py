"""The engine's plan, pinned: for a list of (graph, engine options) configurations, what LoadModel planned (launch order, fused-away operators,
concat aliases, arena footprint, lanes) and which kernel every step of one forward ran.  tests/test_gpu_plan_snapshot.py compares both with the
record tests/golden/plan_snapshot.json, so a planner change that moves a fusion to another layer or packs the arena differently shows up as a list
diff where the count-based assertions of the other suites would still pass.

    python tests/plan_snapshot.py --write      regenerates the record (on a GPU, from a library whose plans are known good)

The record is one JSON line per configuration."""
import atexit
import json
import os
import shutil
import sys
import tempfile

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "plan_snapshot.json")
SCHEDULE_KEYS = ("run", "fused", "alias", "arena_bytes", "per_operand_bytes", "lanes")


# ---- graphs -----------------------------------------------------------------------------------------------------------------------------------
def _tail(tail):
    """the graphs of test_gpu_engine.py::test_fp16_graph_output_from_a_non_conv_layer: an fp32 graph output written by a layer that does not
    convert in its own epilogue (InsertOutputCasts)"""
    def build(mg):
        b = mg.PnnxBuilder(0)
        x = b.input((2, 3, 66, 66))
        y = mg._Conv(b, x, 32, 6, 2)
        if tail == "maxpool":
            y = b.maxpool(y, 5, 1, 2)
        elif tail == "cat":
            y = b.cat([mg._Conv(b, y, 32, 1), b.maxpool(y, 3, 1, 1)], 1)
        elif tail == "add":
            y = b.add(y, mg._Conv(b, y, 32, 3))
        elif tail == "upsample":
            y = b.upsample(y, 2.0)
        b.output(y)
        return b
    return build


def _odd12(mg):
    """a 3x3 conv over 12 channels has no fp16 kernel (test_gpu_engine.py::test_fp16_layers_without_an_fp16_kernel_run_in_fp32_between_casts):
    with fp16 storage it runs in fp32 between the serial-numbered cast steps of InsertFp32Fallbacks"""
    b = mg.PnnxBuilder(1)
    x = b.input((2, 3, 32, 32))
    y = mg._Conv(b, mg._Conv(b, x, 32, 3, 2), 12, 1, 1)
    b.output(mg._Conv(b, mg._Conv(b, y, 24, 3, 1), 16, 1, 1))
    return b


def _conv_transpose_act(mg):
    """nn.ConvTranspose2d -> activation, as test_gpu_conv_transpose.py builds it"""
    b = mg.PnnxBuilder(seed=5)
    x = b.input((2, 32, 10, 14))
    b.output(b.relu(b.conv_transpose(x, 48, (3, 3), (2, 2), (1, 1), (1, 1), (1, 1))))
    return b


def _norms_act(mg):
    """nn.GroupNorm -> activation and nn.InstanceNorm2d -> activation, as test_gpu_groupnorm.py builds them"""
    b = mg.PnnxBuilder(seed=5)
    x = b.input((2, 24, 12, 10))
    y = b.silu(b.group_norm(x, 3))
    b.output(b.leaky_relu(b.instance_norm(y), 0.1))
    return b


def _pool_chain(mg):
    """the SPPF-shaped chain the fused pool kernel does not take (test_gpu_engine.py::test_pool_chain_falls_back_to_three_pools, shape (12, 6))"""
    b = mg.PnnxBuilder(0)
    x = b.input((2, 6, 12, 12))
    y1 = b.maxpool(x, 5, 1, 2)
    y2 = b.maxpool(y1, 5, 1, 2)
    y3 = b.maxpool(y2, 5, 1, 2)
    b.output(b.cat([x, y1, y2, y3], 1))
    return b


# name -> (builder(modelgen), input shape NHWC); the first five are test_gpu_engine.py::MODELS
GRAPHS = {
    "toy_yolo": (lambda mg: mg.build_toy_yolo(2, 64), (2, 64, 64, 3)),
    "toy_classifier": (lambda mg: mg.build_toy_classifier(2, 32), (2, 32, 32, 3)),
    "resnet18_small": (lambda mg: mg.build_resnet18(2, 64, num_classes=100, base=16), (2, 64, 64, 3)),
    "yolov5s_160": (lambda mg: mg.build_yolov5s(2, 160), (2, 160, 160, 3)),
    "mobilenetv3_small_96": (lambda mg: mg.build_mobilenetv3_small(2, 96, num_classes=100), (2, 96, 96, 3)),
    "yolov5s_160_b4": (lambda mg: mg.build_yolov5s(4, 160), (4, 160, 160, 3)),
    "odd12": (_odd12, (2, 32, 32, 3)),
    "conv_transpose_act": (_conv_transpose_act, (2, 10, 14, 32)),
    "norms_act": (_norms_act, (2, 12, 10, 24)),
    "pool_chain_12_6": (_pool_chain, (2, 12, 12, 6)),
}
TAILS = {"silu_unfused": dict(fp16=1, fuse=0), "maxpool": dict(fp16=1), "cat": dict(fp16=1), "add": dict(fp16=1, fuse=0), "upsample": dict(fp16=1)}
for _t in TAILS:
    GRAPHS["tail_" + _t] = (_tail(_t), (2, 66, 66, 3))
MODELS = ("mobilenetv3_small_96", "resnet18_small", "toy_classifier", "toy_yolo", "yolov5s_160")


class Config:
    def __init__(self, graph, **options):
        self.graph, self.options = graph, options
        self.id = "-".join([graph] + ["%s=%d" % kv for kv in options.items()])


CONFIGS = ([Config(m) for m in MODELS] + [Config(m, fuse=0, alias_cat=0) for m in MODELS] +
           [Config("yolov5s_160", **o) for o in (dict(fuse_upsample=0), dict(detect_stream=2), dict(arena=0), dict(fp16=1), dict(fp16=1, fuse_stem=0),
                                                 dict(fp16=1, fuse_stem=1), dict(fp16=1, fuse_pw=0), dict(fp16=1, fuse_pw=2))] +
           [Config("yolov5s_160_b4", streams=2), Config("resnet18_small", fp16=1), Config("mobilenetv3_small_96", fp16=1), Config("odd12", fp16=1)] +
           [Config("tail_" + t, **o) for t, o in TAILS.items()] +
           [Config("conv_transpose_act"), Config("norms_act"), Config("pool_chain_12_6")])
IDS = [c.id for c in CONFIGS]
assert len(set(IDS)) == len(IDS)


# ---- collecting -------------------------------------------------------------------------------------------------------------------------------
_files = {}     # graph name -> (param path, bin path): every graph is generated and saved once per process
_dir = []


def _model_files(si, graph):
    if graph not in _files:
        if not _dir:
            _dir.append(tempfile.mkdtemp(prefix="plan_snapshot_"))
            atexit.register(shutil.rmtree, _dir[0], True)
        pp, bp = (os.path.join(_dir[0], graph + ext) for ext in (".pnnx.param", ".pnnx.bin"))
        GRAPHS[graph][0](si.modelgen).save(pp, bp)
        _files[graph] = (pp, bp)
    return _files[graph]


def _load(si, cfg):
    e = si.Engine(**cfg.options)
    e.load_model(*_model_files(si, cfg.graph))
    return e


def collect_schedule(si, cfg):
    """LoadModel only: nothing is launched"""
    sch = _load(si, cfg).schedule()
    return {k: sch[k] for k in SCHEDULE_KEYS}


def collect_kernels(si, cfg):
    """one forward on the synthetic input, then the kernel of every step"""
    e = _load(si, cfg)
    e.input(e.input_names()[0], si.modelgen.synth_input(GRAPHS[cfg.graph][1]))
    e.forward()
    return [L["kernel"] for L in e.profile()]


def load_record(path=GOLDEN):
    with open(path) as f:
        return json.load(f)


def write_record(si, path=GOLDEN):
    lines = []
    for cfg in CONFIGS:
        rec = dict(schedule=collect_schedule(si, cfg), kernels=collect_kernels(si, cfg))
        lines.append("%s: %s" % (json.dumps(cfg.id), json.dumps(rec, separators=(",", ":"))))
        print("recorded", cfg.id, flush=True)
    with open(path, "w") as f:
        f.write("{\n" + ",\n".join(lines) + "\n}\n")


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import simpleinfer_amd
    if "--write" not in sys.argv:
        sys.exit("usage: python tests/plan_snapshot.py --write")
    write_record(simpleinfer_amd)
    print("wrote", GOLDEN)
