"""GPU: the batch-split modes of the engine -- option "host_slices" (auto from batch 8 on, and explicit), option "streams" = 2 and
ShardedEngine -- on graphs of the operator families no split mode had run, and on graphs that must not be split at all.

A split mode runs pieces of the batch through the model re-batched to N / G.  That is the model's result only when every operator is
per-image (csrc/host/batch_rule.h, tests/test_batch_rule_cpu.py).  Two sets of graphs, all at batch 8 with maps of about 12 x 12 (auto needs
a batch >= 8 that is a multiple of 4: the smallest batch at which every mode is live):

  BATCH-MIXING graphs (a softmax, a reduction, slices and a concatenation over the batch, a batch that is not dimension 0 of the output, a view
  that folds it): every mode must serve them UNSPLIT -- the torch float64 evaluation of the file within util.assert_parity, the bits of the
  engine with host_slices=1 streams=1, schedule() saying host_slices 1 and naming the layer in batch_mixing; streams=2 is kUnsupport at LoadModel.
  Image i carries an offset of i, so the halves of the batch differ in mean by 4 and a slice-wise result is far outside the bar:
  test_split_halves_are_far_outside_the_bar checks exactly that with the float64 evaluator alone (no device), so that the GPU test cannot
  pass on a sliced answer.

  PER-IMAGE graphs, one per operator family: every mode must really split them (host_slices 2 / 2 / 4 slices, lanes 2) and give the bits of the
  unsplit engine, which matches float64.

The reference of every mode is twofold: the same file unsplit (bits) and, independently of the engine, the family's eval_graph in float64.
Every check prints its figures before it asserts (run with -s)."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import act_reference as actr
import attention_reference as ar
import containment as ct
import ct_reference as ctr
import gn_reference as gr
import layout_reference as lr
import pad_reference as padr
import pool_reference as poolr
import reduce_reference as rr
import slice_reference as slr
import softmax_reference as sr
import superres_reference as supr
import up_reference as upr
import util
from simpleinfer_amd import modelgen as mg
from simpleinfer_amd.engine import Engine, Status, StatusError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 8
UNSPLIT = dict(host_slices=1, streams=1)
# the split modes and the slices / lanes a per-image graph of batch 8 must report under them
SPLIT_MODES = {"auto": ({}, 2, 1), "host_slices2": (dict(host_slices=2), 2, 1), "host_slices4": (dict(host_slices=4), 4, 1),
               "streams2": (dict(streams=2), 1, 2)}


class Case:
    """build(n): the PnnxBuilder graph at batch n; ev: the family's float64 evaluator; shape: the NHWC (or [N, F]) input of one image set"""

    def __init__(self, cid, build, ev, shape, lo=-1.0, hi=1.0, offset=False, stored=None, must_differ=True):
        self.id, self.build, self.ev, self.shape, self.lo, self.hi, self.offset = cid, build, ev, tuple(shape), lo, hi, offset
        self.stored = stored or (lambda a: a)      # evaluator's result -> the engine's storage order
        self.must_differ = must_differ

    @functools.lru_cache(maxsize=None)
    def input(self):
        x = util.rng_uniform(31, (N,) + self.shape, self.lo, self.hi)
        if self.offset:   # image i + i: the two halves of the batch differ in mean by 4
            x = (x + np.arange(N, dtype=np.float32).reshape((N,) + (1,) * len(self.shape))).astype(np.float32)
        x.setflags(write=False)
        return x

    @functools.lru_cache(maxsize=None)
    def ref64(self, rnd=None):
        """the float64 evaluation of the batch-8 file: computed once, shared, never written to"""
        r = np.ascontiguousarray(self.stored(self.ev(self.build(N), self.input(), **({"rnd": rnd} if rnd else {}))))
        r.setflags(write=False)
        return r

    def halves64(self):
        """what a 2-slice split computes: the file re-batched to 4 on each half of the batch, the results side by side in the output buffer"""
        x = self.input()
        parts = [np.ascontiguousarray(self.stored(self.ev(self.build(N // 2), x[h * (N // 2):(h + 1) * (N // 2)]))).reshape(-1) for h in (0, 1)]
        return np.concatenate(parts).reshape(self.ref64().shape)


# ---- batch-mixing graphs -------------------------------------------------------------------------------------------------------------------
def softmax0(typ, shape_file_tail, dim):
    def build(n):
        b = mg.PnnxBuilder(seed=5)
        b.output(b.softmax(b.input((n,) + shape_file_tail), dim, functional=typ.startswith("F."), log="og" in typ))
        return b
    return build


def sub_batch_mean(n):
    b = mg.PnnxBuilder(seed=5)
    x = b.input((n, 6, 5, 7))
    b.output(b.expression("sub(@0,@1)", [x, b.mean(x, 0, True)]))
    return b


def div_batch_amax(n):
    b = mg.PnnxBuilder(seed=5)
    x = b.input((n, 6, 5, 7))
    b.output(b.expression("div(@0,@1)", [x, b.amax(x, (0, 2, 3), True)]))
    return b


def conv_softmax0_conv(n):
    b = mg.PnnxBuilder(seed=5)
    x = b.conv(b.input((n, 4, 9, 11)), 6, 3)
    b.output(b.conv(b.softmax(x, 0), 4, 3))
    return b


def swap_halves(n):
    b = mg.PnnxBuilder(seed=5)
    x = b.input((n, 6, 5, 7))
    b.output(b.cat([b.slice(x, 0, n // 2, n), b.slice(x, 0, 0, n // 2)], 0))
    return b


def permute_batch_out(n):
    b = mg.PnnxBuilder(seed=5)
    b.output(b.permute(b.input((n, 8, 5, 6)), (1, 0, 2, 3)))      # C == 8: at batch 8 the output's shape is the input's
    return b


def fold_unfold(n):
    b = mg.PnnxBuilder(seed=5)
    x = b.input((n, 6, 5, 7))
    b.output(b.view(b.sigmoid(b.view(x, (1, n * 6, 5, 7))), (n, 6, 5, 7)))
    return b


lr_eval = lambda b, x: lr.eval_graph(b, x)
MIXING = [
    Case("softmax_dim0_rank4", softmax0("nn.Softmax", (6, 5, 7), 0), sr.eval_graph, (5, 7, 6), offset=True),
    Case("log_softmax_dim0_rank4", softmax0("nn.LogSoftmax", (6, 5, 7), 0), sr.eval_graph, (5, 7, 6), offset=True),
    Case("softmax_dim0_rank2", softmax0("F.softmax", (10,), 0), sr.eval_graph, (10,), offset=True),
    Case("log_softmax_dim0_rank2", softmax0("F.log_softmax", (10,), -2), sr.eval_graph, (10,), offset=True),
    Case("sub_batch_mean", sub_batch_mean, rr.eval_graph, (5, 7, 6), offset=True),
    Case("div_batch_amax", div_batch_amax, rr.eval_graph, (5, 7, 6), 0.0, 1.0, offset=True),
    Case("conv_softmax_dim0_conv", conv_softmax0_conv, sr.eval_graph, (9, 11, 4), offset=True),
    Case("swap_halves", swap_halves, slr.eval_graph, (5, 7, 6), offset=True),
    Case("permute_batch_to_dim1_output", permute_batch_out, lr_eval, (5, 6, 8), offset=True, stored=lr.stored),
    # (an element-wise operator between the two views: whichever way the engine serves this file the values are the same, so it has to match
    # float64 and nothing else is asked of it)
    Case("fold_sigmoid_unfold", fold_unfold, lr_eval, (5, 7, 6), offset=True, stored=lr.stored, must_differ=False),
]
MIXING_IDS = [c.id for c in MIXING]


# ---- per-image graphs, one per operator family ---------------------------------------------------------------------------------------------
def norms(n):
    b = mg.PnnxBuilder(seed=3)
    x = b.relu(b.group_norm(b.conv(b.input((n, 4, 9, 11)), 8, 3), 2))
    b.output(b.conv(b.instance_norm(x, affine=True), 4, 1))
    return b


def pads(n):
    b = mg.PnnxBuilder(seed=3)
    x = b.conv(b.pad(b.input((n, 3, 6, 7)), 1, "reflect"), 4, 3, 1, 0)
    x = b.pad(b.pad(x, (1, 2, 0, 1), "replicate"), 1, "circular")
    x = b.pad(b.pad(x, (1, 0, 1, 0), "constant", 0.5, functional=True), 1, "constant")
    b.output(b.tanh(b.conv(x, 4, 3, 1, 0)))
    return b


def pools(n):
    b = mg.PnnxBuilder(seed=3)
    x = b.relu(b.conv(b.input((n, 4, 12, 12)), 8, 3))
    x = b.adaptive_avgpool(b.avgpool(x, 3, 2, 1), (2, 2))
    b.output(b.linear(b.flatten(x), 10))
    return b


def softmax_dims(n):
    b = mg.PnnxBuilder(seed=3)
    x = b.conv(b.input((n, 4, 6, 7)), 6, 3)
    x = b.softmax2d(b.log_softmax(b.softmax(b.softmax(x, 1), 2), 3, functional=True))
    b.output(b.conv(x, 4, 1))
    return b


def superres(n):
    b = mg.PnnxBuilder(seed=3)
    x = b.prelu(b.conv(b.input((n, 4, 5, 6)), 8, 3), 8)
    x = b.pixel_unshuffle(b.conv(b.pixel_shuffle(x, 2), 4, 3), 2)
    b.output(b.conv(b.prelu(x), 4, 1))
    return b


def reduces(n):
    b = mg.PnnxBuilder(seed=3)
    y = b.relu(b.conv(b.input((n, 4, 7, 9)), 8, 3))
    z = b.mul(y, b.sigmoid(b.mean(y, (2, 3), True)))                 # a per-image channel vector
    o = b.expression("sub(@0,@1)", [z, b.amax(z, 1, True)])          # a per-pixel maximum over the channels
    b.output(b.conv(o, 4, 1))
    return b


def channel_pieces(n):
    b = mg.PnnxBuilder(seed=3)
    a, c = b.chunk(b.conv(b.input((n, 4, 6, 7)), 8, 3), 2, 1)
    d, e = b.split(a, (1, 3), 1)
    b.output(b.conv(b.cat([e, b.slice(c, 1, 1, 3), d], 1), 4, 1))
    return b


def permute_view(n):
    b = mg.PnnxBuilder(seed=3)
    x = b.relu(b.conv(b.input((n, 4, 5, 6)), 6, 3))
    b.output(b.view(b.permute(x, (0, 2, 3, 1)), (n, -1, 3)))
    return b


def conv_transpose(n):
    b = mg.PnnxBuilder(seed=3)
    x = b.relu(b.conv(b.input((n, 4, 5, 6)), 8, 3))
    b.output(b.conv(b.relu(b.conv_transpose(x, 6, 2, 2)), 4, 3))
    return b


def bilinear(n):
    b = mg.PnnxBuilder(seed=3)
    x = b.conv(b.input((n, 4, 5, 6)), 6, 3)
    b.output(b.conv(b.upsample(x, 2.0, "bilinear", align_corners=False), 4, 3))
    return b


def param_acts(n):
    b = mg.PnnxBuilder(seed=3)
    x = b.conv(b.input((n, 4, 6, 7)), 8, 3)
    x = b.mish(b.softplus(b.clamp(b.hardtanh(b.relu6(x), -0.5, 0.8), -0.3, 0.6)))
    b.output(b.conv(x, 4, 1))
    return b


def flatten_linear(n):
    b = mg.PnnxBuilder(seed=3)
    b.output(b.linear(b.flatten(b.relu(b.conv(b.input((n, 4, 5, 6)), 6, 3))), 10))
    return b


PER_IMAGE = [
    Case("groupnorm_instancenorm", norms, gr.eval_graph, (9, 11, 4)),
    Case("pads", pads, padr.eval_graph, (6, 7, 3)),
    Case("avgpool_adaptive", pools, poolr.eval_graph, (12, 12, 4)),
    Case("softmax_dims_1_2_3_softmax2d", softmax_dims, sr.eval_graph, (6, 7, 4)),
    Case("pixelshuffle_prelu", superres, supr.eval_graph, (5, 6, 4)),
    Case("reduce_hw_and_channels", reduces, rr.eval_graph, (7, 9, 4)),
    Case("chunk_split_slice_channels", channel_pieces, slr.eval_graph, (6, 7, 4)),
    Case("permute_view", permute_view, lr_eval, (5, 6, 4), stored=lr.stored),
    Case("conv_transpose", conv_transpose, ctr.eval_graph, (5, 6, 4)),
    Case("bilinear_upsample", bilinear, upr.eval_graph, (5, 6, 4)),
    Case("param_activations", param_acts, actr.eval_graph, (6, 7, 4)),
    # seq-first tokens [L, N, E] behind flatten(2) + permute(2, 0, 1): the batch is dimension 1 through the attention layers
    Case("attention_seq_first_c3tr", lambda n: mg.build_toy_c3tr(n, 24, 32, 4, 1), ar.eval_graph, (24, 24, 3), 0.0, 1.0),
    Case("attention_batch_first_head", lambda n: mg.build_toy_mhsa_head(n, 16), ar.eval_graph, (16, 16, 3), 0.0, 1.0),
    Case("flatten_linear", flatten_linear, sr.eval_graph, (5, 6, 4)),
]
PER_IMAGE_IDS = [c.id for c in PER_IMAGE]


# ---- CPU: the tests below cannot pass on a sliced answer ------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", MIXING, ids=MIXING_IDS)
def test_split_halves_are_far_outside_the_bar(case):
    """float64 evaluator alone: the file evaluated on the two halves of the batch separately fails assert_parity against the file evaluated on
    all 8 images (the folded view around an element-wise operator is the one graph for which both are the same, and is only held to float64)"""
    pytest.importorskip("torch")
    whole, halves = case.ref64(), case.halves64()
    e = util.rel_err(halves, whole)
    print("%s: halves vs whole batch, max|diff|/max|ref| = %.3e" % (case.id, e))
    if not case.must_differ:
        assert e == 0.0
        return
    assert e > 100 * util.REL_TOL, (case.id, e)
    with pytest.raises(AssertionError):
        util.assert_parity(halves, whole, what=case.id)


def test_every_family_of_the_issue_has_a_graph():
    """the operator types the per-image graphs hold, and what the batch-mixing ones do to the batch"""
    types = {ln.split()[0] for c in PER_IMAGE for ln in c.build(N).lines}
    want = {"nn.GroupNorm", "nn.InstanceNorm2d", "nn.ReflectionPad2d", "nn.ReplicationPad2d", "nn.CircularPad2d", "F.pad", "nn.ZeroPad2d", "nn.AvgPool2d",
            "nn.AdaptiveAvgPool2d", "nn.Softmax", "F.log_softmax", "nn.Softmax2d", "nn.PixelShuffle", "nn.PixelUnshuffle", "nn.PReLU", "torch.mean",
            "torch.amax", "torch.chunk", "torch.split", "Tensor.slice", "Tensor.permute", "Tensor.view", "nn.ConvTranspose2d", "nn.Upsample", "nn.ReLU6",
            "nn.Hardtanh", "torch.clamp", "nn.Softplus", "nn.Mish", "nn.MultiheadAttention", "torch.flatten", "nn.Linear"}
    assert want <= types, sorted(want - types)
    assert len(MIXING) == 10 and all(c.input().shape[0] == N for c in MIXING + PER_IMAGE)


# ---- engine helpers -------------------------------------------------------------------------------------------------------------------------
def save(b, tmp_path, tag="m"):
    pp, bp = str(tmp_path / (tag + ".pnnx.param")), str(tmp_path / (tag + ".pnnx.bin"))
    b.save(pp, bp)
    return pp, bp


def serve(pp, bp, x, **opts):
    """LoadModel, then Input / Forward / Extract the reference's way (host tensors) twice: with graph=1 the second forward replays the captured
    graph.  Returns (both outputs, schedule() after the last forward)."""
    e = Engine(**opts)
    e.load_model(pp, bp)
    iname, oname = e.input_names()[0], e.output_names()[0]
    outs = []
    for _ in range(2):
        e.input(iname, x)
        e.forward()
        outs.append(e.extract(oname))
    return outs, e.schedule()


def status_of_load(pp, bp, **opts):
    try:
        Engine(**opts).load_model(pp, bp)
    except StatusError as ex:
        return ex.status
    return Status.kSuccess


# ---- 1. batch-mixing graphs ------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("graph", [0, 1], ids=["eager", "hipgraph"])
@pytest.mark.parametrize("case", MIXING, ids=MIXING_IDS)
def test_batch_mixing_graph_is_served_unsplit(gpu, tmp_path, case, graph):
    pp, bp = save(case.build(N), tmp_path)
    x, ref = case.input(), case.ref64()
    (base, base2), _ = serve(pp, bp, x, graph=graph, **UNSPLIT)
    rows = [("unsplit", base, None)]
    for mode in ("auto", "host_slices2", "host_slices4"):
        (y, y2), sched = serve(pp, bp, x, graph=graph, **SPLIT_MODES[mode][0])
        rows += [(mode, y, sched), (mode + ", second forward", y2, sched)]
    streams = status_of_load(pp, bp, graph=graph, streams=2)
    for mode, y, sched in rows:
        print("%s graph=%d %-30s vs float64 %.3e, elements off the unsplit engine's bits %d, host_slices %s, batch_mixing %s" % (
            case.id, graph, mode, util.rel_err(y, ref), int((y.view(np.uint32) != base.view(np.uint32)).sum()),
            None if sched is None else sched.get("host_slices"), None if sched is None else sched.get("batch_mixing")))
    print("%s graph=%d streams=2: LoadModel -> %s" % (case.id, graph, getattr(streams, "name", streams)))
    ct.assert_same_bits(base2, base, "unsplit, second forward")
    for mode, y, sched in rows:
        what = "%s graph=%d %s" % (case.id, graph, mode)
        util.assert_parity(y, ref, what=what)
        if not case.must_differ:
            continue
        ct.assert_same_bits(y, base, what + " vs the unsplit engine")
        if sched is not None:
            assert sched["host_slices"] == 1, (what, sched["host_slices"])
            assert sched["batch_mixing"] and all(len(m.split(" ", 1)) == 2 for m in sched["batch_mixing"]), (what, sched["batch_mixing"])
    if case.must_differ:
        assert streams == Status.kUnsupport, streams


# ---- 2. per-image graphs ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("graph", [0, 1], ids=["eager", "hipgraph"])
@pytest.mark.parametrize("case", PER_IMAGE, ids=PER_IMAGE_IDS)
def test_per_image_graph_keeps_its_bits_in_every_split_mode(gpu, tmp_path, case, graph):
    pp, bp = save(case.build(N), tmp_path)
    x, ref = case.input(), case.ref64()
    (base, base2), sched0 = serve(pp, bp, x, graph=graph, **UNSPLIT)
    rows = []
    for mode, (opts, slices, lanes) in SPLIT_MODES.items():
        (y, y2), sched = serve(pp, bp, x, graph=graph, **opts)
        rows += [(mode, y, sched, slices, lanes), (mode + ", second forward", y2, sched, slices, lanes)]
    print("%s graph=%d unsplit vs float64 %.3e (element-wise %.3e)" % (case.id, graph, util.rel_err(base, ref), util.mixed_err(base, ref)))
    for mode, y, sched, _, _ in rows:
        print("%s graph=%d %-30s elements off the unsplit engine's bits %d of %d, host_slices %s, lanes %s, batch_mixing %s" % (
            case.id, graph, mode, int((y.view(np.uint32) != base.view(np.uint32)).sum()), y.size, sched.get("host_slices"), sched.get("lanes"),
            sched.get("batch_mixing")))
    util.assert_parity(base, ref, what="%s graph=%d unsplit" % (case.id, graph))
    ct.assert_same_bits(base2, base, "unsplit, second forward")
    assert sched0["host_slices"] == 1 and sched0["lanes"] == 1 and sched0["batch_mixing"] == [], sched0
    for mode, y, sched, slices, lanes in rows:
        what = "%s graph=%d %s" % (case.id, graph, mode)
        assert sched["batch_mixing"] == [], (what, sched["batch_mixing"])
        assert sched["host_slices"] == slices and sched["lanes"] == lanes, (what, sched["host_slices"], sched["lanes"])   # it really was split
        ct.assert_same_bits(y, base, what + " vs the unsplit engine")


# ---- 3. fp16 storage -------------------------------------------------------------------------------------------------------------------------
# graphs whose families' evaluators have the fp16-storage emulation (rnd=): the bar is the one of the sibling files' fp16 toy tests, the error
# against float64 at most twice that of the emulation (weights, input and every stored intermediate rounded to fp16, float64 arithmetic between)
F16_CASES = [(MIXING[6], True), (PER_IMAGE[0], False), (PER_IMAGE[3], False), (PER_IMAGE[8], False)]


@pytest.mark.gpu
@pytest.mark.parametrize("case,mixing", F16_CASES, ids=[c.id for c, _ in F16_CASES])
def test_fp16_storage_in_the_split_modes(gpu, tmp_path, case, mixing):
    pp, bp = save(case.build(N), tmp_path)
    x, ref = case.input(), case.ref64()
    assert case.build(N).lines[-2].split()[0] == "nn.Conv2d"     # (the graph output is fp32 from the conv's own epilogue: no rounding of it)
    emu = case.ref64(sr.round_f16)
    (base, _), _ = serve(pp, bp, x, fp16=1, **UNSPLIT)
    e_engine, e_emu = util.rel_err(base, ref), util.rel_err(emu, ref)
    print("%s fp16 unsplit vs float64: engine %.3e, fp16 emulation %.3e" % (case.id, e_engine, e_emu))
    results = []
    for mode in ("auto", "host_slices4", "streams2"):
        opts, slices, lanes = SPLIT_MODES[mode]
        for graph in (0, 1):
            if mixing and mode == "streams2":
                results.append((mode, graph, status_of_load(pp, bp, fp16=1, graph=graph, streams=2), None))
                continue
            (y, y2), sched = serve(pp, bp, x, fp16=1, graph=graph, **opts)
            results.append((mode, graph, y2, sched))
            print("%s fp16 %s graph=%d: elements off the unsplit engine's bits %d, host_slices %s, lanes %s" % (
                case.id, mode, graph, int((y2.view(np.uint32) != base.view(np.uint32)).sum()), sched.get("host_slices"), sched.get("lanes")))
    assert np.isfinite(base).all() and e_engine <= 2.0 * e_emu, (e_engine, e_emu)
    for mode, graph, y, sched in results:
        what = "%s fp16 %s graph=%d" % (case.id, mode, graph)
        if sched is None:
            assert y == Status.kUnsupport, (what, y)
            continue
        ct.assert_same_bits(y, base, what + " vs the unsplit fp16 engine")
        _, slices, lanes = SPLIT_MODES[mode]
        assert (sched["host_slices"], sched["lanes"], bool(sched["batch_mixing"])) == ((1, 1, True) if mixing else (slices, lanes, False)), (what, sched)


# ---- 4. re-batch alone is not a split ----------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_rebatch_of_a_batch_softmax_is_a_model_of_8_images(gpu, tmp_path):
    """SetOption("batch", 8) on the batch-2 file of softmax(dim=0): a softmax over 8 images, which is what the file means at batch 8"""
    case = MIXING[0]
    pp, bp = save(case.build(2), tmp_path)
    (y, _), sched = serve(pp, bp, case.input(), batch=N)
    print("re-batched 2 -> 8: vs float64 %.3e, host_slices %s" % (util.rel_err(y, case.ref64()), sched.get("host_slices")))
    util.assert_parity(y, case.ref64(), what="softmax(dim=0), batch-2 file served at batch 8")
    assert sched["host_slices"] == 1 and sched["batch_mixing"]


# ---- 5. sharding -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_sharded_engine_refuses_a_batch_mixing_graph(gpu, tmp_path):
    """ShardedEngine::Init (tests/cpp/test_shard_batch_mixing.cpp, one process per rank, the ranks sharing the device as in test_gpu_shard.py):
    two ranks -> kUnsupport on both, before either waits for the other; one rank -> served, and the gathered tensor is the float64 result.  The
    Python twin, ShardedForward, refuses the same way."""
    from simpleinfer_amd import launch, shard
    case = MIXING[0]
    pkg = os.path.join(ROOT, "simpleinfer_amd")
    exe = str(tmp_path / "test_shard_batch_mixing")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "test_shard_batch_mixing.cpp"),
                           "-L" + pkg, "-lsimpleinfer_amd", "-lsi_hip", "-Wl,-rpath," + pkg, "-o", exe])
    pp, bp = save(case.build(N), tmp_path)
    xin = str(tmp_path / "in.f32")
    case.input().tofile(xin)
    for world in (2, 1):
        out = str(tmp_path / ("gathered%d.f32" % world))
        code, text = launch.spawn_ranks([exe, "/si_test_mixing_%d_%d" % (os.getpid(), world), pp, bp, xin, out], world, timeout=120)
        lines = [open(out + ".rank%d" % r).read().strip() for r in range(world) if os.path.exists(out + ".rank%d" % r)]
        print(code, lines)
        assert code == 0 and len(lines) == world, (code, text, lines)
        if world == 2:
            assert lines == ["rank %d of 2: mixing 1 init %d forward -1" % (r, int(Status.kUnsupport)) for r in range(2)], lines
            assert not os.path.exists(out)
        else:
            assert lines == ["rank 0 of 1: mixing 1 init 0 forward 0"], lines
            util.assert_parity(np.fromfile(out, np.float32).reshape(case.ref64().shape), case.ref64(), what="world=1 ShardedEngine")

    class TwoRanks:
        world = 2

    e = Engine(outputs_to_host=0)
    e.load_model(pp, bp)
    with pytest.raises(StatusError) as ei:
        shard.ShardedForward(e, e.output_names()[0], TwoRanks(), 0)
    assert ei.value.status == Status.kUnsupport
