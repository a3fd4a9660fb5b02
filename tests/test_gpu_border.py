"""GPU: the border-mapped convolution (include/si_border.h) and nn.Conv2d(padding_mode = reflect | replicate | circular): the op over the
case table of tests/border_reference.py, exactness, the bit-for-bit invariants, views, the layer on both of its paths, the toy generator
whose convolutions carry the mode, and the refusals at LoadModel."""
import numpy as np
import pytest

import border_reference as br
import containment as ct
import pad_reference as pr
import util
import xcorr_reference as xr
from simpleinfer_amd import hipops, modelgen as mg
from simpleinfer_amd.engine import Engine, Status, StatusError
from test_gpu_f16 import F16_TOL

pytestmark = pytest.mark.gpu

F32, F16 = np.float32, np.float16
MODES = ("reflect", "replicate", "circular")
KEY = "si_hip_conv2d_border"


def kname(dtype):
    return "conv_border_kernel<%s>" % ("_Float16" if np.dtype(dtype) == F16 else "float")


def run(case, x, w, b, **kw):
    """torch layouts in and out"""
    s, p, d, mode = case[6:]
    return br.nchw(hipops.conv2d_border(br.nhwc(x), w, b, br.pair(s), br.pair(p), br.pair(d), mode, half=x.dtype == F16, **kw))


def ref(case, x, w, b, **kw):
    s, p, d, mode = case[6:]
    return br.conv2d_border_ref(x, w, b, s, p, d, mode, **kw)


def same_bits(got, want, what):
    ct.assert_same_bits(np.ascontiguousarray(got), np.ascontiguousarray(want), what)


# ---- the op -----------------------------------------------------------------------------------------------------------------------
OP_CASES = [(c, F32) for c in br.CASES] + [(c, F16) for c in br.F16_CASES]


@pytest.mark.parametrize("case,dtype", OP_CASES, ids=["%s_%s" % (np.dtype(t).name, br.case_id(c)) for c, t in OP_CASES])
def test_op_against_float64(gpu, case, dtype):
    """fp32 at the project's fp32 bar; fp16 storage against the rounding restatement at the fp16 bar"""
    x, w, b = br.operands(case, dtype=dtype)
    got, want = run(case, x, w, b), ref(case, x, w, b, rnd=br.round_f16 if dtype == F16 else None)
    assert hipops.LAST_KERNEL_NAME[KEY] == kname(dtype) and got.shape == want.shape and got.dtype == dtype
    print("border %s %s: max|d| / max|ref| = %.3e" % (np.dtype(dtype).name, br.case_id(case), util.rel_err(got.astype(F32), want)))
    util.assert_parity(got.astype(F32), want, F16_TOL if dtype == F16 else util.REL_TOL, what="border " + br.case_id(case))


@pytest.mark.parametrize("dtype", [F32, F16], ids=["f32", "f16"])
@pytest.mark.parametrize("mode", MODES)
def test_one_hot_filter_is_the_mapped_pixel(gpu, mode, dtype):
    """filter o is 1 at (channel perm[o], tap (ky[o], kx[o])): y[n, o, oy, ox] is the pixel numpy's pad puts at (oy + ky, ox + kx), bit for bit --
    a wrong table entry, tap order or lane map cannot pass.  Small integers; 24 filters over 8 channels, two tiles each way, stride (1, 2)"""
    c, oc, h, wd, kh, kw, ph, pw = 8, 24, br.TH + 1, 2 * br.TW + 4, 3, 5, 1, 2
    r = np.random.Generator(np.random.Philox(3))
    perm, ky, kx = r.integers(0, c, oc), r.integers(0, kh, oc), r.integers(0, kw, oc)
    w = np.zeros((oc, c, kh, kw), F32)
    w[np.arange(oc), perm, ky, kx] = 1.0
    x = r.integers(-64, 65, (2, c, h, wd)).astype(dtype)
    got = run((2, c, h, wd, oc, (kh, kw), (1, 2), (ph, pw), 1, mode), x, w, None)
    xp = np.pad(x, ((0, 0), (0, 0), (ph, ph), (pw, pw)), br.NP_MODE[mode])
    wo = (wd + 2 * pw - kw) // 2 + 1
    want = np.stack([xp[:, perm[o], ky[o]:ky[o] + h, kx[o]:kx[o] + 2 * wo - 1:2] for o in range(oc)], axis=1)
    same_bits(got, want, "one-hot filters, " + mode)


@pytest.mark.parametrize("dtype", [F32, F16], ids=["f32", "f16"])
def test_bits_depend_on_the_image_and_the_filter_alone(gpu, dtype):
    case = (3, br.KC + 8, br.TH + 1, br.TW + 1, br.OCB + 1, 3, 1, 1, 1, "reflect")
    x, w, b = br.operands(case, seed=7, dtype=dtype)
    full = run(case, x, w, b, act1="silu")
    same_bits(run(case, x, w, b, act1="silu"), full, "two runs")
    for i in range(3):
        same_bits(run(case, x[i:i + 1], w, b, act1="silu"), full[i:i + 1], "image %d alone" % i)
    for sel in (slice(17, 18), slice(3, 40), slice(br.OCB, br.OCB + 1)):     # another tile position, another instance of the kernel
        same_bits(run(case, x, w[sel], b[sel], act1="silu"), full[:, sel], "filters %s alone" % (sel,))


VIEWS = {"aligned": dict(in_ld=24, in_c_off=8, res_ld=32, res_c_off=8, out_ld=40, out_c_off=16),     # the 16-byte paths
         "odd": dict(in_ld=13, in_c_off=5, res_ld=23, res_c_off=3, out_ld=25, out_c_off=5)}           # the element paths


@pytest.mark.parametrize("dtype", [F32, F16], ids=["f32", "f16"])
@pytest.mark.parametrize("view", sorted(VIEWS))
def test_views_nan_between_pixels_and_a_sentinel_around_the_output(gpu, view, dtype):
    case = (2, 8, br.TH + 1, br.TW + 1, 20, 3, 1, 1, 1, "circular")
    x, w, b = br.operands(case, seed=11, dtype=dtype)
    res = br.operands((2, 20) + case[2:], seed=12, dtype=dtype)[0]
    kw = dict(act1="relu", residual=br.nhwc(res), act2="relu")
    dense = run(case, x, w, b, **kw)
    v = VIEWS[view]
    for byte in ct.PATTERNS:
        with hipops.guard_bands(byte):
            wide = run(case, x, w, b, in_fill=hipops.ByteFill(0xFF), res_fill=hipops.ByteFill(0xFF), out_fill=hipops.ByteFill(byte), full=True, **kw, **v)
        got = ct.checked_dest(br.nhwc(wide), v["out_c_off"], 20, byte, "%s view under 0x%02X" % (view, byte))
        assert np.isfinite(got).all()
        same_bits(br.nchw(got), dense, "%s view against the dense run" % view)


# ---- the layer --------------------------------------------------------------------------------------------------------------------
def save(b, tmp_path, tag):
    pp, bp = str(tmp_path / (tag + ".pnnx.param")), str(tmp_path / (tag + ".pnnx.bin"))
    b.save(pp, bp)
    return pp, bp


def run_engine(b, tmp_path, x_nhwc, tag="m", forwards=1, **opts):
    e = Engine(**opts)
    e.load_model(*save(b, tmp_path, tag))
    e.input(e.input_names()[0], x_nhwc)
    for _ in range(forwards):
        e.forward()
    return e, e.extract(e.output_names()[0])


def conv_kernels(e):
    return [L["kernel"] for L in e.profile() if L["type"] == "nn.Conv2d"]


def one_op(case, groups=1):
    n, c, h, wd, oc, k, s, p, d, mode = case
    b = mg.PnnxBuilder(seed=4)
    b.output(b.conv(b.input((n, c, h, wd)), oc, br.pair(k), br.pair(s), br.pair(p), br.pair(d), groups=groups, padding_mode=mode))
    return b, b.attrs["conv_0.weight"], b.attrs["conv_0.bias"]


@pytest.mark.parametrize("mode", MODES)
def test_engine_one_op_graph(gpu, tmp_path, mode):
    """LoadModel -> Forward -> Extract equals the op-level call bit for bit and float64 at the bar (zero padding fails this at every border pixel)"""
    case = (2, 8, 9, br.TW + 3, 20, 3, 1, 1, 1, mode)
    b, w, bias = one_op(case)
    x = br.operands(case, seed=21)[0]
    e, got = run_engine(b, tmp_path, br.nhwc(x))
    assert conv_kernels(e) == [kname(F32)], e.profile()
    same_bits(br.nchw(got), run(case, x, w, bias), "engine against the op, " + mode)
    util.assert_parity(br.nchw(got), ref(case, x, w, bias), what="engine one-op graph, " + mode)
    _, cap = run_engine(b, tmp_path, br.nhwc(x), forwards=3, graph=1)
    same_bits(cap, got, "captured over three forwards, " + mode)


def test_engine_fused_relu_and_residual(gpu, tmp_path):
    b = mg.PnnxBuilder(seed=5)
    a = b.relu(b.conv(b.input((2, 3, 9, 11)), 8, 3, 1, 1))
    b.output(b.relu(b.add(a, b.relu(b.conv(a, 8, 3, 1, 1, padding_mode="reflect")))))
    x = br.operands((2, 3, 9, 11, 8, 3), seed=22)[0]
    e, got = run_engine(b, tmp_path, br.nhwc(x))
    types = [L["type"] for L in e.profile()]
    assert conv_kernels(e)[1] == kname(F32) and "nn.ReLU" not in types and "pnnx.Expression" not in types, e.profile()   # one launch: nothing left unfused
    a64 = np.maximum(xr.conv2d_ref(x, b.attrs["conv_0.weight"], b.attrs["conv_0.bias"], 1, 1, 1), 0.0)
    want = np.maximum(a64 + np.maximum(br.conv2d_border_ref(a64, b.attrs["conv_1.weight"], b.attrs["conv_1.bias"], 1, 1, 1, "reflect"), 0.0), 0.0)
    util.assert_parity(br.nchw(got), want, what="conv + relu + residual + relu")


@pytest.mark.parametrize("case,groups,opts", [((2, 8, 9, 11, 8, 3, 1, 1, 1, "reflect"), 4, {}), ((2, 3, 9, 11, 16, 3, 1, 1, 1, "replicate"), 1, dict(fp16=1))],
                         ids=["grouped", "ic3_fp16"])
def test_engine_composition_path(gpu, tmp_path, case, groups, opts):
    """what the kernel does not serve runs as the pad kernel and the layer's ordinary route, and meets the reference"""
    b, w, bias = one_op(case, groups)
    x = br.operands(case, seed=23)[0]
    e, got = run_engine(b, tmp_path, br.nhwc(x), **opts)
    (name,) = conv_kernels(e)
    assert name.startswith("pad2d_kernel + ") and "border" not in name, e.profile()
    util.assert_parity(br.nchw(got), br.conv2d_border_ref(x, w, bias, 1, 1, 1, case[-1], groups=groups), F16_TOL if opts else util.REL_TOL, what="composition")


def test_toy_generator_with_mode_carrying_convolutions(gpu, tmp_path):
    """the in_conv spelling computes the function of the pad-layer spelling: fp32 at the bar, graph=1 the same bits, re-batched the same bits per
    image, and under fp16 storage an error against float64 of at most 2x that of the fp16-storage emulation (test_toy_unet_fp16_storage's rule)"""
    b, spelled = mg.build_toy_cyclegan(base=4, in_conv=True), mg.build_toy_cyclegan(base=4)   # the residual blocks at 16 channels: the kernel's class
    x = mg.synth_input((2, 32, 32, 3))
    want = pr.eval_graph(spelled, x)
    e, got = run_engine(b, tmp_path, x)
    util.assert_parity(got, want, what="toy generator, convolutions carry the mode")
    assert conv_kernels(e).count(kname(F32)) == 4 and len([k for k in conv_kernels(e) if k.startswith("pad2d_kernel + ")]) == 2, e.profile()
    _, cap = run_engine(b, tmp_path, x, forwards=3, graph=1)
    same_bits(cap, got, "graph=1 against eager")
    x3 = np.concatenate([x, x[:1] * 0.5], 0)
    _, y3 = run_engine(b, tmp_path, x3, batch=3)
    same_bits(y3[:2], got, "re-batched, images 0 and 1")
    same_bits(y3[2:], run_engine(b, tmp_path, x3[1:], tag="pair")[1][1:], "re-batched, image 2")
    e16, got16 = run_engine(b, tmp_path, x, fp16=1)
    e_engine, e_emu = util.rel_err(got16, want), util.rel_err(pr.eval_graph(spelled, x, rnd=pr.round_f16), want)
    print("toy generator fp16 storage vs fp64: engine %.3e, fp16 emulation %.3e; kernels %s" % (e_engine, e_emu, conv_kernels(e16)))
    assert conv_kernels(e16).count(kname(F16)) == 4 and np.isfinite(got16).all() and e_engine <= 2.0 * e_emu, (e_engine, e_emu)


@pytest.mark.parametrize("mode,pad", [("reflect", 4), ("circular", 5)])
def test_load_refuses_pads_torch_raises_for(gpu, tmp_path, mode, pad):
    b, _, _ = one_op((1, 8, 4, 4, 8, 2 * pad + 1, 1, pad, 1, mode))
    with pytest.raises(StatusError) as ex:
        Engine().load_model(*save(b, tmp_path, "bad"))
    assert ex.value.status == Status.kUnsupport
    ok, _, _ = one_op((1, 8, 4, 4, 8, 3, 1, 1, 1, mode))      # the process is still usable
    assert np.isfinite(run_engine(ok, tmp_path, np.ones((1, 4, 4, 8), F32), tag="ok")[1]).all()
