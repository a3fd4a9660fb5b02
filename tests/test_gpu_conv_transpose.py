"""GPU: nn.ConvTranspose2d -- si_hip_conv_transpose2d_f32 against the fp64 scatter-form reference (tests/ct_reference.py), and the layer
inside the engine: one-op graphs, activation fusion, a toy U-Net in fp32 and with fp16 storage, and the files the engine refuses."""
import numpy as np
import pytest

import util
from ct_reference import SHAPES, conv_transpose2d_ref, eval_graph, operands, round_f16, shape_id, _parse
from simpleinfer_amd import hipops, modelgen as mg
from simpleinfer_amd.engine import Engine, Status, StatusError

pytestmark = pytest.mark.gpu


def run_op(s, act="none", act_param=0.0, bias=True, **kw):
    k, st, p, op, d, _, _ = s
    x, w, b = operands(s)
    got = hipops.conv_transpose2d(x, w, b if bias else None, st, p, op, d, act1=act, act_param=act_param, **kw)
    ref = conv_transpose2d_ref(x, w, b if bias else None, st, p, op, d, act=act, act_param=act_param)
    return got, ref


@pytest.mark.parametrize("s", SHAPES, ids=[shape_id(s) for s in SHAPES])
def test_op_matches_reference(gpu, s):
    got, ref = run_op(s)
    print("%s: max-based %.3e, element-wise %.3e" % (shape_id(s), util.rel_err(got, ref), util.mixed_err(got, ref)))
    util.assert_parity(got, ref, what=shape_id(s))


ODD = [((2, 2), (2, 2), (0, 0), (0, 0), (1, 1), (2, 9, 7), (3, 1)),
       ((3, 3), (2, 2), (1, 1), (1, 1), (1, 1), (2, 6, 5), (17, 5)),
       ((2, 2), (2, 2), (0, 0), (0, 0), (1, 1), (1, 5, 6), (1, 255)),
       ((3, 3), (2, 2), (1, 1), (0, 0), (1, 1), (1, 4, 4), (1, 255))]


@pytest.mark.parametrize("s", ODD, ids=[shape_id(s) for s in ODD])
def test_odd_channel_counts(gpu, s):
    got, ref = run_op(s)
    util.assert_parity(got, ref, what=shape_id(s))


@pytest.mark.parametrize("k", [(2, 2, 0, 0), (3, 2, 1, 1)], ids=["k2s2", "k3s2p1op1"])
def test_batch5_without_bias(gpu, k):
    kk, ss, pp, op = k
    s = ((kk, kk), (ss, ss), (pp, pp), (op, op), (1, 1), (5, 7, 6), (24, 40))
    got, ref = run_op(s, bias=False)
    util.assert_parity(got, ref, what="n5 no bias")


@pytest.mark.parametrize("act,param", [("relu", 0.0), ("silu", 0.0), ("leakyrelu", 0.1), ("sigmoid", 0.0), ("hardswish", 0.0)])
@pytest.mark.parametrize("si", [0, 2], ids=["one_tap", "phases"])
def test_activations(gpu, act, param, si):
    got, ref = run_op(SHAPES[si], act=act, act_param=param)
    util.assert_parity(got, ref, what=act)


@pytest.mark.parametrize("si", [0, 2, 8], ids=["one_tap", "phases", "k3x2"])
def test_strided_views(gpu, si):
    """input at in_ld = Cin + 8 with NaN between the pixels' channels; output into channels [off, off + Cout) of a wider buffer pre-filled with a
    sentinel: every channel outside the view keeps the sentinel bit for bit"""
    s = SHAPES[si]
    x, w, b = operands(s)
    ci, co = s[6]
    sentinel = np.float32(-12345.678)
    off, ld = 12, co + 20
    k, st, p, op, d = s[:5]
    y = hipops.conv_transpose2d(x, w, b, st, p, op, d, in_ld=ci + 8, in_fill=np.nan, out_ld=ld, out_c_off=off, out_fill=float(sentinel), full=True)
    ref = conv_transpose2d_ref(x, w, b, st, p, op, d)
    util.assert_parity(y[..., off:off + co], ref, what="strided view")
    outside = np.concatenate([y[..., :off], y[..., off + co:]], axis=-1)
    assert np.array_equal(outside.view(np.uint32), np.full(outside.shape, sentinel, np.float32).view(np.uint32))


@pytest.mark.parametrize("si", [0, 1, 4], ids=["one_tap", "one_tap_1024", "k4s2p1"])
def test_same_bits_twice(gpu, si):
    a, _ = run_op(SHAPES[si])
    b, _ = run_op(SHAPES[si])
    util.assert_exact(a.view(np.uint32), b.view(np.uint32), "two launches")


# ---- engine ---------------------------------------------------------------------------------------------------------------------------------
def save(b, tmp_path, tag="m"):
    pp, bp = str(tmp_path / (tag + ".pnnx.param")), str(tmp_path / (tag + ".pnnx.bin"))
    b.save(pp, bp)
    return pp, bp


def run_engine(pp, bp, x, **opts):
    e = Engine(**opts)
    e.load_model(pp, bp)
    e.input(e.input_names()[0], x)
    e.forward()
    return e, e.extract(e.output_names()[0])


def one_op_graph(s, act=None):
    k, st, p, op, d, (n, h, w), (ci, co) = s
    b = mg.PnnxBuilder(seed=5)
    x = b.input((n, ci, h, w))
    y = b.conv_transpose(x, co, k, st, p, op, d)
    if act == "relu":
        y = b.relu(y)
    b.output(y)
    return b


@pytest.mark.parametrize("si", [0, 2, 6, 8], ids=["one_tap", "phases", "k1s2", "k3x2"])
def test_engine_one_op_graph(gpu, tmp_path, si):
    """LoadModel -> Forward -> Extract reproduces the op-level result bit for bit (and the reference)"""
    s = SHAPES[si]
    b = one_op_graph(s)
    pp, bp = save(b, tmp_path)
    k, st, p, op, d, (n, h, w), (ci, co) = s
    x = util.rng_uniform(9, (n, h, w, ci), -1.0, 1.0)
    _, got = run_engine(pp, bp, x)
    name = [ln.split()[1] for ln in b.lines if ln.startswith("nn.ConvTranspose2d")][0]
    wt, bias = b.attrs[name + ".weight"], b.attrs[name + ".bias"]
    op_level = hipops.conv_transpose2d(x, wt, bias, st, p, op, d)
    util.assert_exact(got.view(np.uint32), op_level.view(np.uint32), "engine vs op level")
    util.assert_parity(got, conv_transpose2d_ref(x, wt, bias, st, p, op, d), what="engine")


def test_relu_is_fused_into_the_epilogue(gpu, tmp_path):
    s = SHAPES[2]
    b = one_op_graph(s, act="relu")
    pp, bp = save(b, tmp_path)
    k, st, p, op, d, (n, h, w), (ci, co) = s
    x = util.rng_uniform(11, (n, h, w, ci), -1.0, 1.0)
    name = [ln.split()[1] for ln in b.lines if ln.startswith("nn.ConvTranspose2d")][0]
    ref = conv_transpose2d_ref(x, b.attrs[name + ".weight"], b.attrs[name + ".bias"], st, p, op, d, act="relu")
    e1, y1 = run_engine(pp, bp, x, fuse=1)
    e0, y0 = run_engine(pp, bp, x, fuse=0)
    util.assert_parity(y1, ref, what="fuse=1")
    util.assert_parity(y0, ref, what="fuse=0")
    assert "relu_0" in e1.schedule()["fused"] and "relu_0" not in e0.schedule()["fused"]
    p1, p0 = e1.profile(), e0.profile()
    assert len(p1) == len(p0) - 1, (p1, p0)
    assert any(L["type"] == "nn.ConvTranspose2d" and L["kernel"].startswith("conv_transpose_f32_kernel") for L in p1), p1


# ---- toy U-Net ------------------------------------------------------------------------------------------------------------------------------
def unet_files(tmp_path, batch=2):
    b = mg.build_toy_unet(batch=batch)
    return b, save(b, tmp_path, "unet%d" % batch)


def test_toy_unet_fp32(gpu, tmp_path):
    b, (pp, bp) = unet_files(tmp_path)
    x = mg.synth_input((2, 64, 64, 3))
    e, got = run_engine(pp, bp, x)
    ref = eval_graph(b, x)
    print("toy U-Net fp32: max-based %.3e, element-wise %.3e" % (util.rel_err(got, ref), util.mixed_err(got, ref)))
    util.assert_parity(got, ref, what="toy U-Net fp32")
    # each up-conv writes straight into its concat buffer (alias_cat, the default)
    ups = [_parse(ln)[3][0] for ln in b.lines if ln.startswith("nn.ConvTranspose2d")]
    assert len(ups) == 3
    alias = e.schedule()["alias"]
    assert all(u in alias for u in ups), (ups, alias)
    kernels = {L["kernel"] for L in e.profile() if L["type"] == "nn.ConvTranspose2d"}
    assert kernels == {"conv_transpose_f32_kernel<true, true>", "conv_transpose_f32_kernel<false, true>"}, kernels
    # a captured graph replays the same bits
    _, g = run_engine(pp, bp, x, graph=1)
    util.assert_exact(g.view(np.uint32), got.view(np.uint32), "graph=1 vs eager")


def test_toy_unet_rebatch(gpu, tmp_path):
    """SetOption("batch", 5) on the batch-2 file: per image the same bits as batch-2 runs of the same images"""
    b, (pp, bp) = unet_files(tmp_path)
    x5 = util.rng_uniform(21, (5, 64, 64, 3), 0.0, 1.0)
    _, y5 = run_engine(pp, bp, x5, batch=5)
    xs = np.concatenate([x5, x5[:1]], 0)   # pairs (0, 1), (2, 3), (4, 0)
    for i in range(0, 6, 2):
        _, y2 = run_engine(pp, bp, xs[i:i + 2])
        for j in range(2):
            if i + j < 5:
                util.assert_exact(y5[i + j].view(np.uint32), y2[j].view(np.uint32), "image %d" % (i + j))


def test_toy_unet_fp16_storage(gpu, tmp_path):
    """fp16=1: the engine loads, the transposed convs run fp32 between casts, and the error against fp64 is at most 2x that of an fp16-storage
    emulation (weights, biases, the input and every layer's output rounded to fp16, fp64 arithmetic in between) on the same input"""
    b, (pp, bp) = unet_files(tmp_path)
    x = mg.synth_input((2, 64, 64, 3))
    e, got = run_engine(pp, bp, x, fp16=1)
    prof = e.profile()
    ct = [L for L in prof if L["type"] == "nn.ConvTranspose2d"]
    assert len(ct) == 3 and all(L["kernel"].startswith("conv_transpose_f32_kernel") for L in ct), ct
    ref = eval_graph(b, x)
    emu = eval_graph(b, x, rnd=round_f16)
    e_engine, e_emu = util.rel_err(got, ref), util.rel_err(emu, ref)
    print("toy U-Net fp16 storage vs fp64: engine %.3e, fp16 emulation %.3e" % (e_engine, e_emu))
    assert np.isfinite(got).all()
    assert e_engine <= 2.0 * e_emu, (e_engine, e_emu)


def test_refusals_leave_the_process_usable(gpu, tmp_path):
    # groups = 2: kUnsupport
    b = mg.PnnxBuilder()
    x = b.input((1, 8, 6, 6))
    y = b.conv_transpose(x, 8, 2, 2, 0)
    b.output(y)
    b.lines = [ln.replace(" groups=1 ", " groups=2 ") for ln in b.lines]
    name = [ln.split()[1] for ln in b.lines if ln.startswith("nn.ConvTranspose2d")][0]
    w = b.attrs[name + ".weight"]
    b.attrs[name + ".weight"] = np.ascontiguousarray(w[:, :4])
    b.lines = [ln.replace("@weight=(8,8,2,2)f32", "@weight=(8,4,2,2)f32") for ln in b.lines]
    pp, bp = save(b, tmp_path, "groups2")
    with pytest.raises(StatusError) as ei:
        Engine().load_model(pp, bp)
    assert ei.value.status == Status.kUnsupport
    # an output shape that disagrees with the formula: kErrorShape
    b = mg.PnnxBuilder()
    x = b.input((1, 8, 6, 6))
    y = b.conv_transpose(x, 8, 3, 2, 1, output_padding=1)   # (1, 8, 12, 12)
    b.output(y)
    b.lines = [ln.replace("#%s=(1,8,12,12)f32" % y, "#%s=(1,8,11,12)f32" % y) for ln in b.lines]
    pp, bp = save(b, tmp_path, "badshape")
    with pytest.raises(StatusError) as ei:
        Engine().load_model(pp, bp)
    assert ei.value.status == Status.kErrorShape
    # ... and the same process loads and runs a good model afterwards
    s = SHAPES[0]
    pp, bp = save(one_op_graph(s), tmp_path, "good")
    k, st, p, op, d, (n, h, w), (ci, co) = s
    _, out = run_engine(pp, bp, util.rng_uniform(3, (n, h, w, ci), -1.0, 1.0))
    assert out.shape == (n, 2 * h, 2 * w, co) and np.isfinite(out).all()
