"""GPU: nn.GroupNorm / nn.InstanceNorm2d -- si_hip_groupnorm_f32 / _f16 (include/si_norm.h) against the float64 reference
(tests/gn_reference.py): both kernel forms, vector and scalar paths, data with a large common offset, the epilogue activations,
strided views under guard bands, bit-level determinism, the refusals; and the layer inside the engine: one-op graphs, activation
fusion, the toy U-Net with group / instance norm in fp32, under graph capture, re-batched, and with fp16 storage."""
import ctypes as C

import numpy as np
import pytest

import containment as ct
import gn_reference as gr
import util
from ct_reference import _parse
from simpleinfer_amd import _native, hipops, modelgen as mg
from simpleinfer_amd.engine import Engine, Status, StatusError

pytestmark = pytest.mark.gpu

SLAB, TWO = "groupnorm_slab_kernel", "groupnorm_stats_kernel"


def run_op(s, affine=True, eps=1e-5, act="none", act_param=0.0, half=False, offset=0.0, seed=0, **kw):
    """(got, ref, kernel name): the reference is evaluated on the input the kernel saw (rounded to half first for the fp16 entry)"""
    x, gamma, beta = gr.operands(s, seed, offset)
    if half:
        x = x.astype(np.float16)
    g, b = (gamma, beta) if affine else (None, None)
    got = hipops.group_norm(x, s[4], g, b, eps, act1=act, act_param=act_param, half=half, **kw)
    return got, gr.group_norm_ref(x, s[4], g, b, eps, act, act_param), hipops.LAST_KERNEL_NAME["si_hip_groupnorm"]


# ---- op level, fp32 -------------------------------------------------------------------------------------------------------------
KERNELS_SEEN = set()


@pytest.mark.parametrize("variant", ["affine", "plain", "eps1e-3"])
@pytest.mark.parametrize("s", gr.SHAPES + gr.EXTRA_SHAPES, ids=gr.shape_id)
def test_op_matches_reference(gpu, s, variant):
    got, ref, kernel = run_op(s, affine=variant != "plain", eps=1e-3 if variant == "eps1e-3" else 1e-5)
    KERNELS_SEEN.add(kernel.split("<")[0])
    print("%s %s [%s]: max-based %.3e, element-wise %.3e" % (gr.shape_id(s), variant, kernel, util.rel_err(got, ref), util.mixed_err(got, ref)))
    assert got.dtype == np.float32
    util.assert_parity(got, ref, what="%s %s" % (gr.shape_id(s), variant))
    if s == gr.TWO_LAUNCH:
        assert kernel == "groupnorm_stats_kernel<float, 4> + groupnorm_apply_kernel<float, 4>", kernel
        assert hipops.group_norm_workspace_bytes(s[:4], s[4]) > 0
    else:
        assert kernel.startswith(SLAB if s in gr.SHAPES else TWO), kernel


def test_both_forms_ran(gpu):
    """the names reported over the shape list include both forms (runs after the parametrised test above, whose names it collects)"""
    if not KERNELS_SEEN:
        for s in (gr.SHAPES[0], gr.TWO_LAUNCH):
            KERNELS_SEEN.add(run_op(s)[2].split("<")[0])
    assert KERNELS_SEEN >= {SLAB, TWO}, KERNELS_SEEN


@pytest.mark.parametrize("affine", [True, False], ids=["affine", "plain"])
def test_one_element_per_group_is_act_of_beta_bit_for_bit(gpu, affine):
    s = (1, 1, 1, 8, 8)
    x, gamma, beta = gr.operands(s, 3)
    for act in ("none", "relu"):
        got = hipops.group_norm(x * 100.0, 8, gamma if affine else None, beta if affine else None, act1=act)
        want = (beta if affine else np.zeros(8, np.float32)).reshape(1, 1, 1, 8)
        want = np.maximum(want, np.float32(0.0)) if act == "relu" else want
        util.assert_exact(got.view(np.uint32), want.astype(np.float32).view(np.uint32), "act(beta), %s" % act)


# ---- data with a large common offset: the statistics must not cancel -----------------------------------------------------------
@pytest.mark.parametrize("s", gr.OFFSET_SHAPES, ids=gr.shape_id)
def test_offset_30_fp32(gpu, s):
    """x = 30 + U[-1, 1): a float32 emulation of Chan-combined partials is 1.8e-5 .. 2.0e-5 from float64 element-wise on such data, a
    sum-of-squares formulation 2.8e-4 .. 3.9e-4; the bar is the project's 1e-4 on both metrics"""
    got, ref, kernel = run_op(s, offset=30.0, seed=5)
    print("offset 30 %s [%s]: max-based %.3e, element-wise %.3e" % (gr.shape_id(s), kernel, util.rel_err(got, ref), util.mixed_err(got, ref)))
    util.assert_parity(got, ref, what="offset 30 %s" % gr.shape_id(s))


# ---- activations ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("act,param", [("relu", 0.0), ("silu", 0.0), ("leakyrelu", 0.1), ("sigmoid", 0.0), ("hardswish", 0.0)])
@pytest.mark.parametrize("si", [0, 2], ids=["vector", "scalar"])
def test_activations(gpu, act, param, si):
    got, ref, _ = run_op(gr.SHAPES[si], act=act, act_param=param)
    util.assert_parity(got, ref, what=act)


# ---- fp16 -------------------------------------------------------------------------------------------------------------------------
def assert_half_bar(got, ref, what):
    """|got - ref| <= 2^-11 |ref| + 1e-4 max|ref|: one round-to-nearest-even at the store plus the fp32 bar"""
    assert got.dtype == np.float16, got.dtype
    g, r = got.astype(np.float64), np.asarray(ref, np.float64)
    assert np.isfinite(g).all(), what
    bound = 2.0 ** -11 * np.abs(r) + 1e-4 * np.abs(r).max()
    excess = np.abs(g - r) - bound
    print("%s: worst |d| / bound %.3f" % (what, float((np.abs(g - r) / np.maximum(bound, 1e-300)).max())))
    assert (excess <= 0).all(), "%s: %d elements over the bound, worst by %.3e" % (what, int((excess > 0).sum()), float(excess.max()))


@pytest.mark.parametrize("affine", [True, False], ids=["affine", "plain"])
@pytest.mark.parametrize("s", gr.HALF_SHAPES + [gr.TWO_LAUNCH, gr.EXTRA_SHAPES[0]], ids=gr.shape_id)
def test_fp16_matches_reference(gpu, s, affine):
    got, ref, kernel = run_op(s, affine=affine, half=True)
    assert "_Float16" in kernel, kernel
    if s == (2, 10, 6, 21, 3):
        assert kernel.endswith("<_Float16, 1>"), kernel     # the scalar half path
    assert_half_bar(got, ref, "fp16 %s [%s]" % (gr.shape_id(s), kernel))


@pytest.mark.parametrize("s", gr.OFFSET_SHAPES, ids=gr.shape_id)
def test_offset_30_fp16(gpu, s):
    got, ref, kernel = run_op(s, half=True, offset=30.0, seed=5)
    assert_half_bar(got, ref, "fp16 offset 30 %s [%s]" % (gr.shape_id(s), kernel))


# ---- views and containment: checks (a) - (d) of tests/test_gpu_containment.py, the workspace among the guarded buffers -----------------
class ViewCase:
    def __init__(self, cid, entry, s, half, c_pad, out_off, out_ld):
        self.id, self.entries, self.s, self.half = cid, ("si_hip_" + entry,), s, half
        self.in_ld, self.in_off, self.out_off, self.out_ld = s[3] + 8, c_pad, out_off, out_ld

    def run(self, F):
        x, gamma, beta = gr.operands(self.s, 7)
        y = hipops.group_norm(x, self.s[4], gamma, beta, act1="silu", half=self.half, in_ld=self.in_ld, in_c_off=self.in_off, in_fill=F,
                              out_ld=self.out_ld, out_c_off=self.out_off, out_fill=F, full=True)
        return ct.Out("y", y, self.out_off, self.s[3])


VIEW_CASES = []
for _half, _sfx in ((False, "f32"), (True, "f16")):
    VIEW_CASES += [
        ViewCase("vector_" + _sfx, "groupnorm_" + _sfx, (2, 12, 10, 24, 3), _half, 8, 16, 56),     # 16-byte aligned slices on both sides
        ViewCase("scalar_" + _sfx, "groupnorm_" + _sfx, (1, 9, 7, 6, 2), _half, 3, 5, 13),          # odd offsets and strides
        ViewCase("two_launch_" + _sfx, "groupnorm_" + _sfx, gr.TWO_LAUNCH, _half, 8, 8, 48),
    ]


@pytest.mark.parametrize("case", VIEW_CASES, ids=[c.id for c in VIEW_CASES])
def test_views_and_containment(gpu, case):
    del hipops.LAST_ENTRIES[:]
    plain = case.run(hipops.ByteFill(0x00))
    plain_kernel = hipops.LAST_KERNEL_NAME["si_hip_groupnorm"]
    assert set(case.entries) <= set(hipops.LAST_ENTRIES), hipops.LAST_ENTRIES
    assert plain_kernel.startswith(TWO if case.id.startswith("two_launch") else SLAB), plain_kernel
    assert ("1>" in plain_kernel) == case.id.startswith("scalar"), plain_kernel
    ct.assert_outside_fill(plain.full, plain.c_off, plain.c, 0x00, case.id + ", plain run")
    ct.assert_finite(plain.dest, case.id + ", plain run")
    # the value too: the NaN in the input gaps reached no statistic
    x, gamma, beta = gr.operands(case.s, 7)
    if case.half:
        assert_half_bar(np.ascontiguousarray(plain.dest), gr.group_norm_ref(x.astype(np.float16), case.s[4], gamma, beta, act="silu"), case.id)
    else:
        util.assert_parity(plain.dest, gr.group_norm_ref(x, case.s[4], gamma, beta, act="silu"), what=case.id)
    for byte in ct.PATTERNS:
        with hipops.guard_bands(byte) as g:      # (a) all bands and (d) the inputs are compared when the block ends
            out = case.run(hipops.ByteFill(byte))
        what = "%s under 0x%02X" % (case.id, byte)
        want_buffers = 4 + (1 if case.id.startswith("two_launch") else 0)   # gamma, beta, x, y (+ the workspace)
        assert g.checked == want_buffers, "%s: the guard saw %d buffers" % (what, g.checked)
        assert hipops.LAST_KERNEL_NAME["si_hip_groupnorm"] == plain_kernel, what
        ct.assert_outside_fill(out.full, out.c_off, out.c, byte, what)                              # (b)
        ct.assert_same_bits(out.dest, plain.dest, what + ": guarded + pattern-filled vs plain")    # (c)
        ct.assert_finite(out.dest, what)


# ---- determinism ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s", [gr.SHAPES[0], gr.TWO_LAUNCH], ids=["one_launch", "two_launches"])
@pytest.mark.parametrize("half", [False, True], ids=["f32", "f16"])
def test_same_bits_twice(gpu, s, half):
    a, _, _ = run_op(s, half=half)
    b, _, _ = run_op(s, half=half)
    ct.assert_same_bits(a, b, "two launches")


@pytest.mark.parametrize("s", [(5, 12, 10, 24, 3), (5, 48, 40, 32, 4)], ids=gr.shape_id)
@pytest.mark.parametrize("half", [False, True], ids=["f32", "f16"])
def test_batch_of_5_has_the_bits_of_single_images(gpu, s, half):
    x, gamma, beta = gr.operands(s, 11)
    x = x.astype(np.float16) if half else x
    y5 = hipops.group_norm(x, s[4], gamma, beta, half=half)
    for i in range(5):
        y1 = hipops.group_norm(x[i:i + 1], s[4], gamma, beta, half=half)
        ct.assert_same_bits(y5[i:i + 1], y1, "image %d" % i)


# ---- engine ---------------------------------------------------------------------------------------------------------------------------
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


def one_op_graph(s, kind="gn", act=None, affine=True, **kw):
    n, h, w, c, g = s
    b = mg.PnnxBuilder(seed=5)
    x = b.input((n, c, h, w))
    y = b.group_norm(x, g, affine=affine, **kw) if kind == "gn" else b.instance_norm(x, affine=affine, **kw)
    if act == "silu":
        y = b.silu(y)
    b.output(y)
    return b


def norm_params(b):
    name = [ln.split()[1] for ln in b.lines if ln.startswith(("nn.GroupNorm", "nn.InstanceNorm2d"))][0]
    return b.attrs.get(name + ".weight"), b.attrs.get(name + ".bias")


def test_refusals_leave_the_process_usable(gpu, tmp_path):
    x, gamma, beta = gr.operands((1, 4, 4, 8, 2))
    with pytest.raises(hipops.HipError):
        hipops.group_norm(x, 3, gamma, beta)                      # C % G != 0
    d = hipops.group_norm_desc(x.shape, 2, in_ld=7)                # ld < C (the wrapper would not build such a view: the entry itself)
    src, dst = hipops.DeviceBuffer(x.nbytes), hipops.DeviceBuffer(x.nbytes)
    with pytest.raises(hipops.HipError):
        hipops._chk(_native.hip().si_hip_groupnorm_f32(C.byref(d), src.ptr, None, None, dst.ptr, None, None), "si_hip_groupnorm_f32")
    xt, gt, bt = gr.operands(gr.TWO_LAUNCH)
    assert hipops.group_norm_workspace_bytes(xt.shape, 4) > 0
    with pytest.raises(hipops.HipError):
        hipops.group_norm(xt, 4, gt, bt, workspace=False)         # a null workspace where bytes > 0

    def load(b, tag):
        pp, bp = save(b, tmp_path, tag)
        with pytest.raises(StatusError) as ei:
            Engine().load_model(pp, bp)
        return ei.value.status

    assert load(one_op_graph((1, 6, 6, 8, 8), "in", affine=False, track_running_stats=True), "trs") == Status.kUnsupport
    b = one_op_graph((1, 6, 6, 8, 2))
    b.lines = [ln.replace(" num_channels=8 ", " num_channels=16 ") for ln in b.lines]
    assert load(b, "channels") == Status.kErrorShape
    b = one_op_graph((1, 6, 6, 8, 2))
    b.lines = [ln.replace(" num_groups=2 ", " num_groups=3 ") for ln in b.lines]
    assert load(b, "groups") == Status.kErrorShape
    # ... and the same process loads and runs a good model afterwards
    s = (1, 6, 6, 8, 2)
    b = one_op_graph(s)
    pp, bp = save(b, tmp_path, "good")
    x = util.rng_uniform(3, (1, 6, 6, 8), -1.0, 1.0)
    _, out = run_engine(pp, bp, x)
    util.assert_parity(out, gr.group_norm_ref(x, 2, *norm_params(b)), what="good model after the refusals")


@pytest.mark.parametrize("kind,s", [("gn", (2, 12, 10, 24, 3)), ("gn", gr.TWO_LAUNCH), ("in", (2, 16, 16, 64, 64)), ("in", (3, 5, 6, 7, 7))],
                         ids=["gn_one_launch", "gn_two_launches", "in_vector", "in_scalar"])
def test_engine_one_op_graph(gpu, tmp_path, kind, s):
    """LoadModel -> Forward -> Extract reproduces the op-level result bit for bit (and the reference)"""
    b = one_op_graph(s, kind, affine=kind == "gn")
    pp, bp = save(b, tmp_path)
    x = util.rng_uniform(9, s[:4], -1.0, 1.0)
    e, got = run_engine(pp, bp, x)
    gamma, beta = norm_params(b)
    op_level = hipops.group_norm(x, s[4], gamma, beta)
    util.assert_exact(got.view(np.uint32), op_level.view(np.uint32), "engine vs op level")
    util.assert_parity(got, gr.group_norm_ref(x, s[4], gamma, beta), what="engine")
    norm = [L for L in e.profile() if L["type"] in ("nn.GroupNorm", "nn.InstanceNorm2d")]
    assert len(norm) == 1 and norm[0]["kernel"] == hipops.group_norm_kernel_name(s[:4], s[4]), norm
    assert norm[0]["bytes"] == 2.0 * x.nbytes, norm


def test_silu_is_fused_into_the_epilogue(gpu, tmp_path):
    s = gr.TWO_LAUNCH
    b = one_op_graph(s, act="silu")
    pp, bp = save(b, tmp_path)
    x = util.rng_uniform(11, s[:4], -1.0, 1.0)
    ref = gr.group_norm_ref(x, s[4], *norm_params(b), act="silu")
    e1, y1 = run_engine(pp, bp, x, fuse=1)
    e0, y0 = run_engine(pp, bp, x, fuse=0)
    util.assert_parity(y1, ref, what="fuse=1")
    util.assert_parity(y0, ref, what="fuse=0")
    assert "silu_0" in e1.schedule()["fused"] and "silu_0" not in e0.schedule()["fused"]
    p1, p0 = e1.profile(), e0.profile()
    assert len(p1) == len(p0) - 1, (p1, p0)
    name = hipops.group_norm_kernel_name(s[:4], s[4])
    assert [L["kernel"] for L in p1 if L["type"] == "nn.GroupNorm"] == [name], p1
    assert [L["kernel"] for L in p0 if L["type"] == "nn.GroupNorm"] == [name], p0


UNETS = {"gn_silu": dict(norm="gn", act="silu"), "in_relu": dict(norm="in")}
NORM_TYPES = ("nn.GroupNorm", "nn.InstanceNorm2d")


@pytest.mark.parametrize("which", sorted(UNETS))
def test_toy_unet_fp32(gpu, tmp_path, which):
    b = mg.build_toy_unet(**UNETS[which])
    pp, bp = save(b, tmp_path, which)
    x = mg.synth_input((2, 64, 64, 3))
    e, got = run_engine(pp, bp, x)
    ref = gr.eval_graph(b, x)
    print("toy U-Net %s fp32: max-based %.3e, element-wise %.3e" % (which, util.rel_err(got, ref), util.mixed_err(got, ref)))
    util.assert_parity(got, ref, what="toy U-Net %s fp32" % which)
    prof = e.profile()
    norms = [L for L in prof if L["type"] in NORM_TYPES]
    assert len(norms) == 14 and {L["kernel"].split("<")[0] for L in norms} == {SLAB, TWO}, norms   # both forms inside one network
    acts = [ln.split()[1] for ln in b.lines if ln.startswith(("nn.SiLU", "nn.ReLU"))]
    assert set(acts) <= set(e.schedule()["fused"]), e.schedule()["fused"]
    # the up-convs still write straight into their concat buffers, and the norm layers read / write the aliased views
    ups = [_parse(ln)[3][0] for ln in b.lines if ln.startswith("nn.ConvTranspose2d")]
    alias = e.schedule()["alias"]
    assert len(ups) == 3 and all(u in alias for u in ups), (ups, alias)
    # a captured graph replays the same bits
    _, g = run_engine(pp, bp, x, graph=1)
    util.assert_exact(g.view(np.uint32), got.view(np.uint32), "graph=1 vs eager")


@pytest.mark.parametrize("which", sorted(UNETS))
def test_toy_unet_rebatch(gpu, tmp_path, which):
    """SetOption("batch", 5) on the batch-2 file: per image the same bits as batch-2 runs of the same images"""
    b = mg.build_toy_unet(**UNETS[which])
    pp, bp = save(b, tmp_path, which)
    x5 = util.rng_uniform(21, (5, 64, 64, 3), 0.0, 1.0)
    _, y5 = run_engine(pp, bp, x5, batch=5)
    xs = np.concatenate([x5, x5[:1]], 0)   # pairs (0, 1), (2, 3), (4, 0)
    for i in range(0, 6, 2):
        _, y2 = run_engine(pp, bp, xs[i:i + 2])
        for j in range(2):
            if i + j < 5:
                util.assert_exact(y5[i + j].view(np.uint32), y2[j].view(np.uint32), "image %d" % (i + j))


@pytest.mark.parametrize("which", sorted(UNETS))
def test_toy_unet_fp16_storage(gpu, tmp_path, which):
    """fp16=1: every norm layer runs the fp16 kernel on half tensors with no cast pair around it, and the error against fp64 is at most 2x
    that of the fp16-storage emulation (weights, biases, the input and every layer's output rounded to fp16, fp64 arithmetic between)"""
    b = mg.build_toy_unet(**UNETS[which])
    pp, bp = save(b, tmp_path, which)
    x = mg.synth_input((2, 64, 64, 3))
    e, got = run_engine(pp, bp, x, fp16=1)
    prof = e.profile()
    norms = [L for L in prof if L["type"] in NORM_TYPES]
    assert len(norms) == 14 and all("_Float16" in L["kernel"] for L in norms), norms
    names = [L["name"] for L in prof]
    for L in norms:   # (InsertFp32Fallbacks names its casts <layer>.in_to_f32.<k> / <layer>.out_to_f16.<k>)
        assert not any(n.startswith(L["name"] + ".in_to_f32") or n.startswith(L["name"] + ".out_to_f16") for n in names), names
    ref = gr.eval_graph(b, x)
    emu = gr.eval_graph(b, x, rnd=gr.round_f16)
    e_engine, e_emu = util.rel_err(got, ref), util.rel_err(emu, ref)
    print("toy U-Net %s fp16 storage vs fp64: engine %.3e, fp16 emulation %.3e" % (which, e_engine, e_emu))
    assert np.isfinite(got).all()
    assert e_engine <= 2.0 * e_emu, (e_engine, e_emu)
