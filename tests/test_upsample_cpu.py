"""CPU: bilinear nn.Upsample / F.interpolate, size= and the label map -- the numpy reference pinned to torch, the conditions of the
GPU tests (fp16 bound, fair label-map inputs, reachable engine bar), the C-ABI entry points that need no device, and the generator."""
import ctypes as C
import hashlib
import os

import numpy as np
import pytest

import up_reference as ur
import util
from simpleinfer_amd import _native, engine, hipops, modelgen as mg

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
REF_BIN = os.path.join(ROOT, "oracle", "_ref", "ref_pnnx_dump")

ALL_CASES = [(s, ac, ur.form_args(s, f)) for s, ac, f in ur.BASE_CASES] + [(s, ac, kw) for s, kw in ur.EXTRA_CASES for ac in (False, True)]


def torch_interpolate(torch, x_nhwc, mode, ac, kw, channels_last=False, recompute=None):
    t = torch.from_numpy(np.ascontiguousarray(x_nhwc)).permute(0, 3, 1, 2)
    t = t.contiguous(memory_format=torch.channels_last) if channels_last else t.contiguous()
    args = dict(size=tuple(kw["out_hw"])) if "out_hw" in kw else dict(scale_factor=kw["scale"], recompute_scale_factor=recompute)
    if mode == "bilinear":
        args["align_corners"] = ac
    y = torch.nn.functional.interpolate(t, mode=mode, **args)
    return y.permute(0, 2, 3, 1).contiguous().numpy()


# ---- 1. the reference is torch's rule ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,ac,kw", ALL_CASES, ids=[ur.case_id(*c) for c in ALL_CASES])
def test_reference_equals_torch_fp32(shape, ac, kw):
    """max|torch - ref| <= 8 * 2^-24 * max|x|: torch's float32 blend is five roundings, each <= 2^-24 of a magnitude <= max|x|, rounded
    up to a power of two; the coordinates are the same floats by construction"""
    torch = pytest.importorskip("torch")
    x = ur.case_input(shape)
    ref = ur.upsample_bilinear_ref(x, align_corners=ac, **kw)
    for cl in (False, True):
        got = torch_interpolate(torch, x, "bilinear", ac, kw, cl)
        assert got.shape == ref.shape and got.dtype == np.float32
        err = float(np.abs(got.astype(np.float64) - ref).max())
        print("%s %s: %.2f x 2^-24 max|x|" % (ur.case_id(shape, ac, kw), "channels-last" if cl else "contiguous",
                                               err / (ur.EPS * np.abs(x).max())))
        assert err <= ur.blend_bound(x)


@pytest.mark.parametrize("shape", ur.BASE_SHAPES, ids=["x".join(map(str, s)) for s in ur.BASE_SHAPES])
def test_recompute_scale_factor_is_the_size_form(shape):
    torch = pytest.importorskip("torch")
    x = ur.case_input(shape, 1)
    for scale in (1.5, 3.7):
        for ac in (False, True):
            got = torch_interpolate(torch, x, "bilinear", ac, dict(scale=scale), recompute=True)
            ref = ur.upsample_bilinear_ref(x, scale=scale, align_corners=ac, recompute=True)
            by_size = ur.upsample_bilinear_ref(x, out_hw=ref.shape[1:3], align_corners=ac)
            assert np.array_equal(ref, by_size)
            assert float(np.abs(got - ref).max()) <= ur.blend_bound(x)


@pytest.mark.parametrize("shape", ur.BASE_SHAPES, ids=["x".join(map(str, s)) for s in ur.BASE_SHAPES])
def test_nearest_by_size_reference_equals_torch(shape):
    torch = pytest.importorskip("torch")
    x = ur.case_input(shape, 2)
    for out_hw in (ur.form_args(shape, "size")["out_hw"], (shape[1] + 3, 2 * shape[2] + 1), (max(1, shape[1] // 2), max(1, shape[2] - 1))):
        got = torch_interpolate(torch, x, "nearest", False, dict(out_hw=out_hw))
        util.assert_exact(got.view(np.uint32), ur.upsample_nearest_ref(x, out_hw=out_hw).view(np.uint32), "nearest to %s" % (out_hw,))


# ---- 2. the fp16 bound holds for torch alone ------------------------------------------------------------------------------
# (shape, align_corners, size / scale, channels-last).  torch's CPU kernel for half tensors has two paths: the vectorised channels-last one
# (c >= 4) and the one small tensors take keep the interpolation weights in float32, as the rule here does; the separable path a wide
# contiguous tensor takes stores coordinates and weights in HALF and misses any fp32-blend bound by two orders of magnitude (measured on
# 1x7x300x3 -> 15x898: 414x this bound contiguous, 0.995x the same data with c = 4 channels-last).  That path is torch's own economy, not
# the rule; the wide-axis case below therefore runs channels-last.
FP16_CASES = [((2, 64, 64, 21), False, dict(out_hw=(512, 512)), False), ((2, 65, 65, 21), True, dict(out_hw=(513, 513)), False),
              ((1, 13, 9, 21), True, dict(scale=3.7), False), ((2, 16, 16, 8), False, dict(scale=2.0), False),
              ((1, 7, 300, 4), True, dict(out_hw=(15, 898)), True)]


def fp16_bound(ref64, x):
    """half an fp16 ulp of the result (one round-to-nearest-even store) plus the fp32 blend error"""
    return 2.0 ** -11 * np.abs(ref64) + ur.blend_bound(x)


@pytest.mark.parametrize("shape,ac,kw,cl", FP16_CASES, ids=[ur.case_id(*c[:3]) for c in FP16_CASES])
def test_fp16_bound_holds_for_torch(shape, ac, kw, cl):
    torch = pytest.importorskip("torch")
    x = ur.case_input(shape, 3, half=True)
    ref = ur.upsample_bilinear_ref(x, align_corners=ac, **kw)
    got = torch_interpolate(torch, x, "bilinear", ac, kw, channels_last=cl)
    assert got.dtype == np.float16
    ratio = np.abs(got.astype(np.float64) - ref) / fp16_bound(ref, x)
    print("%s: worst %.3f of the bound" % (ur.case_id(shape, ac, kw), ratio.max()))
    assert ratio.max() <= 1.0


# ---- 3. the label-map inputs are fair ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("half", [False, True], ids=["fp32", "fp16"])
@pytest.mark.parametrize("case", ur.LABEL_CASES, ids=["seed%d" % c[0] for c in ur.LABEL_CASES])
def test_label_map_inputs_are_fair(case, half):
    """the share of pixels whose two largest reference values are closer than 2 * 8 * 2^-24 * max|x| is at most 2e-4 (the condition of
    the GPU label-map test), and a float32 numpy blend picks the float64 argmax on every other pixel"""
    seed, shape, out_hw, ac = case
    x = ur.label_logits(seed, shape, half)
    labels, near = ur.label_ref(x, out_hw, ac)
    share = near.mean()
    print("seed %d %s: %d / %d near ties (%.2e)" % (seed, "fp16" if half else "fp32", near.sum(), near.size, share))
    assert share <= ur.LABEL_TIE_CAP
    f32 = ur.upsample_bilinear_ref(x, out_hw=out_hw, align_corners=ac, blend=np.float32).argmax(axis=-1)
    assert np.array_equal(f32[~near], labels[~near])


# ---- 4. the C-ABI without a device ----------------------------------------------------------------------------------------------
NEW_SYMBOLS = ("si_upsample_step", "si_upsample_out_size", "si_hip_upsample_bilinear_f32", "si_hip_upsample_bilinear_f16",
               "si_hip_upsample_bilinear_kernel_name", "si_hip_upsample_nearest_steps_f32", "si_hip_segment_labels_f32",
               "si_hip_segment_labels_f16")
BADARG, UNSUPPORTED = -1, -2


def test_abi_without_a_device(native_libs):
    H, _ = native_libs
    for name in NEW_SYMBOLS:
        assert hasattr(H, name), name
    dummy = C.c_void_p(256)
    good = lambda: hipops.upsample_desc((2, 8, 8, 21), out_hw=(64, 64))
    entries = (H.si_hip_upsample_bilinear_f32, H.si_hip_upsample_bilinear_f16, H.si_hip_segment_labels_f32, H.si_hip_segment_labels_f16)

    def bad(**fields):
        d = good()
        for k, v in fields.items():
            setattr(d, k, v)
        return d

    for fields in (dict(n=0), dict(ih=0), dict(iw=-3), dict(c=0), dict(oh=0), dict(ow=-1), dict(in_ld=20), dict(step_h=float("nan")),
                   dict(step_w=float("inf")), dict(step_h=-0.5)):
        for fn in entries:
            assert fn(C.byref(bad(**fields)), dummy, dummy, None) == BADARG, (fields, fn)
    for fn in entries[:2]:
        assert fn(C.byref(bad(out_ld=20)), dummy, dummy, None) == BADARG
        assert fn(C.byref(bad(n=4, ih=4096, iw=4096, c=64, in_ld=64, out_ld=64)), dummy, dummy, None) == UNSUPPORTED   # 2^32 elements
        assert fn(C.byref(bad(oh=65536, ow=65536, c=1, in_ld=1, out_ld=1)), dummy, dummy, None) == UNSUPPORTED
        assert fn(None, dummy, dummy, None) == BADARG
    for fn in entries[2:]:
        assert fn(C.byref(bad(c=257, in_ld=257)), dummy, dummy, None) == UNSUPPORTED
    assert H.si_hip_upsample_nearest_steps_f32(dummy, 1, 4, 4, 8, 4, 1.0, 1.0, dummy, 8, 8, 8, None) == BADARG      # ld < c
    assert H.si_hip_upsample_nearest_steps_f32(dummy, 1, 4, 4, 8, 8, float("nan"), 1.0, dummy, 8, 8, 8, None) == BADARG
    assert H.si_hip_upsample_nearest_steps_f32(dummy, 4, 4096, 4096, 64, 64, 1.0, 1.0, dummy, 8, 8, 64, None) == UNSUPPORTED   # 2^32 elements
    assert H.si_hip_upsample_nearest_steps_f32(dummy, 1, 4, 4, 1, 1, 1.0, 1.0, dummy, 65536, 65536, 1, None) == UNSUPPORTED
    # the kernel the engine's profile names: 16 bytes per lane where c and both strides allow it, narrower otherwise
    name = lambda *a, **k: hipops.upsample_bilinear_kernel_name(*a, **k)
    assert name((2, 16, 16, 64), scale=2) == "upsample_bilinear_kernel<float, 4>"
    assert name((2, 16, 16, 21), scale=2) == "upsample_bilinear_kernel<float, 1>"
    assert name((2, 16, 16, 64), scale=2, out_ld=66) == "upsample_bilinear_kernel<float, 1>"
    assert name((2, 16, 16, 64), scale=2, half=True) == "upsample_bilinear_kernel<_Float16, 8>"
    assert name((2, 16, 16, 20), scale=2, half=True) == "upsample_bilinear_kernel<_Float16, 4>"
    assert name((2, 16, 16, 22), scale=2, half=True) == "upsample_bilinear_kernel<_Float16, 2>"
    assert name((2, 16, 16, 21), scale=2, half=True) == "upsample_bilinear_kernel<_Float16, 1>"


def test_host_helper_reproduces_the_rule(native_libs):
    """step values and output sizes written out from the formulas of the rule"""
    H, _ = native_libs
    f = np.float32

    def step(mode, n_in, n_out, ac, scale):
        st = C.c_float(-1.0)
        assert H.si_upsample_step(mode, n_in, n_out, ac, scale, C.byref(st)) == 0
        return f(st.value)

    BIL, NEAR = 1, 0
    table = [
        # mode, in, out, align_corners, scale_factor (0: not given), expected step
        (BIL, 16, 32, 1, 0.0, f(15) / f(31)),
        (BIL, 16, 32, 1, 2.0, f(15) / f(31)),            # align_corners ignores the scale factor
        (BIL, 9, 1, 1, 0.0, f(0)),                       # out = 1
        (BIL, 1, 5, 1, 0.0, f(0)),
        (BIL, 65, 513, 1, 0.0, f(64) / f(512)),
        (BIL, 16, 32, 0, 2.0, f(0.5)),
        (BIL, 300, 1110, 0, 3.7, f(1.0 / 3.7)),
        (BIL, 7, 25, 0, 3.7, f(1.0 / 3.7)),
        (BIL, 7, 25, 0, 0.0, f(7) / f(25)),              # recompute_scale_factor=True: the size form, another step (0.28, not 0.27027)
        (BIL, 13, 19, 0, 1.5, f(1.0 / 1.5)),
        (BIL, 64, 512, 0, 0.0, f(0.125)),
        (BIL, 12, 7, 0, 0.0, f(12) / f(7)),
        (NEAR, 12, 7, 0, 0.0, f(12) / f(7)),
        (NEAR, 7, 300, 0, 0.0, f(7) / f(300)),
        (NEAR, 20, 40, 0, 2.0, f(0.5)),
    ]
    for mode, n_in, n_out, ac, scale, want in table:
        got = step(mode, n_in, n_out, ac, scale)
        assert got.tobytes() == want.tobytes(), (mode, n_in, n_out, ac, scale, got, want)
        # ... and they are the reference's
        ref = ur.axis_step("bilinear" if mode == BIL else "nearest", n_in, n_out, bool(ac), scale or None)
        assert got.tobytes() == f(ref).tobytes()
    st = C.c_float()
    assert H.si_upsample_step(NEAR, 8, 16, 1, 0.0, C.byref(st)) == BADARG      # nearest has no align_corners
    assert H.si_upsample_step(BIL, 0, 16, 0, 0.0, C.byref(st)) == BADARG
    assert H.si_upsample_step(BIL, 8, 16, 0, -2.0, C.byref(st)) == BADARG
    assert H.si_upsample_step(2, 8, 16, 0, 0.0, C.byref(st)) == BADARG
    for n_in, scale, want in ((300, 3.7, 1110), (7, 3.7, 25), (13, 1.5, 19), (9, 1.5, 13), (16, 2.0, 32), (10, 0.5, 5), (5, 1.9, 9), (3, 1.0 / 3.0, 1)):
        assert H.si_upsample_out_size(n_in, scale) == want == ur.out_size(n_in, scale), (n_in, scale)
    assert H.si_upsample_out_size(3, 0.2) == BADARG and H.si_upsample_out_size(3, 0.0) == BADARG   # an empty output
    assert hipops.upsample_out_hw(7, 300, 3.7) == (25, 1110)


# ---- 5. generator and loader --------------------------------------------------------------------------------------------------------
def _digests(b, tmp_path, tag):
    pp, bp = str(tmp_path / (tag + ".pnnx.param")), str(tmp_path / (tag + ".pnnx.bin"))
    b.save(pp, bp)
    return hashlib.sha256(open(pp, "rb").read()).hexdigest(), hashlib.sha256(open(bp, "rb").read()).hexdigest()


def test_existing_generator_output_is_unchanged(tmp_path):
    """digests of the files the generator wrote before it learned the new keywords"""
    b = mg.PnnxBuilder()
    x = b.input((1, 8, 6, 6))
    b.upsample(x)
    b.upsample(x, 3.0)
    assert b.lines[1:] == ["nn.Upsample upsample_0 1 1 0 1 mode=nearest scale_factor=(2.0,2.0) size=None #0=(1,8,6,6)f32 #1=(1,8,12,12)f32",
                           "nn.Upsample upsample_1 1 1 0 2 mode=nearest scale_factor=(3.0,3.0) size=None #0=(1,8,6,6)f32 #2=(1,8,18,18)f32"]
    assert _digests(mg.build_toy_unet(), tmp_path, "a") == ("d7b3b205a90cde8f929b28281f2ae3e24ac4fc6bf9748a4641a10b49b01e7e74",
                                                            "73552b1e535ff098bfc451e173d97147c00040ae035f6ecc6f7a8d7f82a076be")
    assert _digests(mg.build_toy_unet(batch=1, size=32, base=8, depth=2, ncls=3, seed=4), tmp_path, "b") == (
        "a98f12119735aeb3150a1aded9aec3806e7b3fd715b53338cdb4af060a17ddbe", "8e195360f1939d52bbfe2669954f1b0a10d4c14bc19f60dab16e8ee3934e44be")
    assert _digests(mg.build_toy_unet(up="convtranspose"), tmp_path, "c")[0] == "d7b3b205a90cde8f929b28281f2ae3e24ac4fc6bf9748a4641a10b49b01e7e74"
    assert _digests(mg.build_yolov5s(1, 64), tmp_path, "d")[0] == "9df43b268de60e938b3407db5a01e5c93c5daed33761cbe6d3f256c022dc3648"


def test_new_generator_lines():
    b = mg.PnnxBuilder()
    x = b.input((1, 8, 6, 10))
    b.upsample(x, 2.0, mode="bilinear", align_corners=True)
    b.upsample(x, mode="nearest", size=(9, 9))
    b.interpolate(x, scale=1.5, mode="bilinear", align_corners=False, recompute_scale_factor=True)
    b.interpolate(x, mode="bilinear", align_corners=False, size=(64, 64))
    b.interpolate(x, scale=2.0, mode="bilinear", align_corners=True, functional="F.upsample")
    assert b.lines[1:] == [
        "nn.Upsample upsample_0 1 1 0 1 align_corners=True mode=bilinear scale_factor=(2.0,2.0) size=None #0=(1,8,6,10)f32 #1=(1,8,12,20)f32",
        "nn.Upsample upsample_1 1 1 0 2 mode=nearest scale_factor=None size=(9,9) #0=(1,8,6,10)f32 #2=(1,8,9,9)f32",
        "F.interpolate F_interpolate_0 1 1 0 3 align_corners=False mode=bilinear recompute_scale_factor=True scale_factor=(1.5,1.5) size=None "
        "#0=(1,8,6,10)f32 #3=(1,8,9,15)f32",
        "F.interpolate F_interpolate_1 1 1 0 4 align_corners=False mode=bilinear recompute_scale_factor=None scale_factor=None size=(64,64) "
        "#0=(1,8,6,10)f32 #4=(1,8,64,64)f32",
        "F.upsample F_upsample_0 1 1 0 5 align_corners=True mode=bilinear scale_factor=(2.0,2.0) size=None #0=(1,8,6,10)f32 #5=(1,8,12,20)f32"]


BUILDERS = {"unet_bilinear": lambda: mg.build_toy_unet(up="bilinear"), "segnet": lambda: mg.build_toy_segnet()}


@pytest.mark.parametrize("which", sorted(BUILDERS))
def test_new_toy_graphs_load_like_the_reference_loader(native_libs, tmp_path, which):
    b = BUILDERS[which]()
    text = "\n".join(b.lines)
    if which == "unet_bilinear":
        assert text.count("nn.Upsample") == 3 and text.count("align_corners=True mode=bilinear scale_factor=(2.0,2.0)") == 3
        assert "nn.ConvTranspose2d" not in text
    else:
        assert "size=(64,64)" in text and "scale_factor=None" in text and "recompute_scale_factor=None" in text
        assert text.count("F.interpolate") == 2 and "dilation=(2,2)" in text and "scale_factor=(2.0,2.0) size=None" in text
    pp, bp = str(tmp_path / "m.pnnx.param"), str(tmp_path / "m.pnnx.bin")
    b.save(pp, bp)
    import subprocess
    for expand in (False, True):
        out = str(tmp_path / "dump.txt")
        engine.pnnx_dump(pp, bp, expand, out)
        ours = open(out).read()
        assert ("F.interpolate" if which == "segnet" else "nn.Upsample") in ours
        if not os.path.exists(REF_BIN):
            continue
        ref = subprocess.run([REF_BIN, pp, bp] + (["--expand"] if expand else []), check=True, capture_output=True, text=True).stdout
        assert ours == ref
    if not os.path.exists(REF_BIN):
        pytest.skip("oracle/_ref/ref_pnnx_dump is not built here: the product loader read the file, the comparison did not run")


# ---- 6. the engine bar is reachable ---------------------------------------------------------------------------------------------------
def torch_eval(torch, b, x):
    F = torch.nn.functional
    from ct_reference import _ints, _parse
    vals, got = {}, None
    for typ, name, ins, outs, prm in (_parse(ln) for ln in b.lines):
        a = lambda k: torch.from_numpy(b.attrs["%s.%s" % (name, k)])
        if typ == "pnnx.Input":
            vals[outs[0]] = torch.from_numpy(x).permute(0, 3, 1, 2).contiguous()
            continue
        if typ == "pnnx.Output":
            got = vals[ins[0]].permute(0, 2, 3, 1).contiguous().numpy()
            continue
        t = vals[ins[0]]
        if typ == "nn.Conv2d":
            y = F.conv2d(t, a("weight"), a("bias"), stride=_ints(prm["stride"]), padding=_ints(prm["padding"]), dilation=_ints(prm["dilation"]))
        elif typ == "nn.BatchNorm2d":
            y = F.batch_norm(t, a("running_mean"), a("running_var"), a("weight"), a("bias"), False, 0.0, float(prm["eps"]))
        elif typ == "nn.ReLU":
            y = F.relu(t)
        elif typ == "nn.MaxPool2d":
            y = F.max_pool2d(t, 2, 2)
        elif typ == "torch.cat":
            y = torch.cat([vals[i] for i in ins], 1)
        elif typ == "pnnx.Expression":
            y = vals[ins[0]] + vals[ins[1]]
        elif typ in ur.RESIZE_TYPES:
            mode, kw, ac, rec = ur.resize_args(prm)
            args = dict(size=kw["out_hw"]) if "out_hw" in kw else dict(scale_factor=kw["scale"], recompute_scale_factor=rec or None)
            y = F.interpolate(t, mode=mode, align_corners=ac if mode == "bilinear" else None, **args)
        else:
            raise NotImplementedError(typ)
        vals[outs[0]] = y
    return got


@pytest.mark.parametrize("which", sorted(BUILDERS))
def test_toy_graph_fp32_evaluation_is_within_the_bar(which):
    """The condition of the GPU engine tests: a torch float32 CPU evaluation of the graph on synth_input is itself within REL_TOL of the
    float64 evaluation on both metrics, so an fp32 engine can be held to that bar on this graph."""
    torch = pytest.importorskip("torch")
    b = BUILDERS[which]()
    x = mg.synth_input((2, 64, 64, 3))
    ref = ur.eval_graph(b, x)
    got = torch_eval(torch, b, x)
    assert got.dtype == np.float32 and got.shape == ref.shape == (2, 64, 64, 4 if which == "unet_bilinear" else 21)
    e, m = util.rel_err(got, ref), util.mixed_err(got, ref)
    print("torch float32 vs fp64 on %s: max-based %.3e, element-wise %.3e" % (which, e, m))
    assert e <= util.REL_TOL and m <= util.REL_TOL
