"""GPU: fp16 storage on views its kernels refuse.

The planner's concat and split aliasing asks only that a slice starts on a 16-byte boundary; the row (the parent's channel count) may be anything.
The fp16 entries that read or write 16-byte vectors answer SI_E_UNSUPPORTED for a row that is no multiple of 8 halves, and most of the layers
that call them have no second launch.  Every family below is one small graph in which such an entry meets such a row -- ODD is a 1x1 conv to 4
channels placed as a concat piece (rows of 36, 68, 132 halves), TWIN the same graph with ODD widened to 8 channels, the control that the route
under test is really the one the graph takes.  Each case asserts: the graph is the one intended (offsets, widths, the fp32 alias); the twin's fp16
profile shows the kernel; fp16 loads and runs twice; the raw bits are those of the same engine with every operand dense (alias_cat = 0,
alias_split = 0) -- eager, replayed as a hipGraph over four forwards, with arena = 0, and (against its own dense run) with fuse = 0; no more cast
steps than the twin; the error against fp64 is at most 2x that of the fp16-storage emulation; and the fp32 engine matches its plain schedule.

What the engine does with these graphs: before an alias is made every step that touches the operand is asked whether its launch takes the row
(Layer::TakesView, csrc/host/view_rule.h); a declined alias is the copy the concat or split launches anyway.  Deviations from the shapes the
families were first sketched with, each because the sketched shape does not take the route:
  * G (upsampled source) has 128 + 128 -> 128 channels: the fp16 dual-source form reads whole K blocks (64 channels when ic % 64 == 0), and
    f32_split takes a dual-source 1x1 layer from K = 256 and 128 output columns on.
  * the f32_split checks of B and G use rows of 3 extra channels and wide layers: a row of 64 + 4 FLOATS is whole 16-byte vectors, which the
    split kernels take, and f32_split takes sibling-fused 1x1 layers only from K = 256 with 256 output columns on.  G's upsampled source at such
    a row is declined at load in fp32 too (si_hip_conv2d_upcat_f32 has no second launch either), so that layer stays on the split kernel and
    is held to the parity bar, not to equal bits.
"""
import numpy as np
import pytest

import slice_reference as ref
import util
from util import assert_exact, assert_parity

pytestmark = pytest.mark.gpu

ODD, TWIN = 4, 8


@pytest.fixture(scope="module")
def si(gpu):
    import simpleinfer_amd
    return simpleinfer_amd


def _save(tmp_path, builder, tag):
    pp, bp = str(tmp_path / (tag + ".pnnx.param")), str(tmp_path / (tag + ".pnnx.bin"))
    builder.save(pp, bp)
    return pp, bp


def _engine(si, pp, bp, x, forwards=1, **opts):
    """load, then `forwards` forwards: the engine and the output of each"""
    e = si.Engine(**opts)
    e.load_model(pp, bp)
    (iname,), (oname,) = e.input_names(), e.output_names()
    e.input(iname, x)
    outs = []
    for _ in range(forwards):
        e.forward()
        outs.append(e.extract(oname))
    return e, outs


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _casts(e):
    return [n for n in e.schedule()["run"] if ".in_to_f32." in n or ".out_to_f16." in n]


def _kernels(e):
    return {L["name"]: L["kernel"] for L in e.profile()}


# ---- the families: build(mg, w) with w the ODD / TWIN channel count.  `piece`: (operand, channel offset, parent width) of the aliased piece;
# `route(kernels, schedule, profile)`: the twin's fp16 engine takes the route under test; `layers`: steps that must have no cast pair around them
def fam_a(mg, w):
    b = mg.PnnxBuilder(seed=11)
    x = b.input((2, 16, 8, 16))
    p = b.silu(b.conv(x, 32, 1))                 # conv_0
    o = b.conv(x, w, 1)                          # conv_1: ODD
    a = b.silu(b.conv(p, 32, 3))                 # conv_2 reads p at the concat's row: si_hip_conv2d_f16, in_ld 68
    b.output(b.cat([p, o, a]))
    return dict(b=b, shape=(2, 8, 16, 16), piece=(p, 0, 64 + w), layers=["conv_2"], route=lambda k, s, prof: "f16" in k["conv_2"])


def fam_b(mg, w, c=32, c1=32, c2=64):
    b = mg.PnnxBuilder(seed=12)
    x = b.input((2, 16, 8, 16))
    p = b.silu(b.conv(x, c, 1))                  # conv_0
    o = b.conv(x, w, 1)                          # conv_1: ODD
    u = b.silu(b.conv(p, c1, 1))                 # conv_2 | conv_3: one launch (CanFuseSibling), si_hip_conv2d_split_f16
    v = b.silu(b.conv(p, c2, 1))
    b.output(b.cat([p, o, u, v]))
    return dict(b=b, shape=(2, 8, 16, 16), piece=(p, 0, c + w + c1 + c2), layers=["conv_2"],
                route=lambda k, s, prof: "f16" in k["conv_2"] and "conv_3" in s["fused"] and "conv_3" not in s["run"])


def fam_c1(mg, w, c=32, h=8):
    b = mg.PnnxBuilder(seed=13)
    x = b.input((2, 16, h, 16))
    p = b.silu(b.conv(x, c, 1))                  # conv_0: the pair's input and shortcut
    o = b.conv(x, w, 1)                          # conv_1: ODD
    m = b.silu(b.conv(p, c, 1))                  # conv_2: folded into conv_3's launch (the patch form of si_hip_conv2d_pw_slab_f16)
    q = b.add(b.silu(b.conv(m, c, 3)), p)        # conv_3
    b.output(b.cat([p, o, q]))
    return dict(b=b, shape=(2, h, 16, 16), piece=(p, 0, 2 * c + w), layers=["conv_3"],
                route=lambda k, s, prof: k["conv_3"] == "conv_pw_patch_f16_kernel<pw + 3x3>" and "conv_2" in s["fused"])


def fam_c2(mg, w):
    b = mg.PnnxBuilder(seed=14)
    x = b.input((32, 16, 40, 40))
    p = b.silu(b.conv(x, 128, 1))                # conv_0
    m = b.silu(b.conv(p, 128, 1))                # conv_1: folded into conv_2's launch (the slab form)
    a = b.silu(b.conv(m, 128, 3))                # conv_2 writes the first piece of a 132-wide concat: slab out_ld 132
    q = b.add(a, p)
    o = b.conv(x, w, 1)                          # conv_3: ODD
    b.output(b.cat([q, o]))
    q = "pnnx_expr_0_add(%s,%s)" % (a, p)        # (expression lowering renames the operand on the engine side)
    return dict(b=b, shape=(32, 40, 40, 16), piece=(q, 0, 128 + w), layers=["conv_2"], opts=dict(host_slices=1), ref_images=2,
                route=lambda k, s, prof: k["conv_2"] == "conv3x3s1_slab_f16_kernel<pw + 3x3>" and "conv_1" in s["fused"])


def fam_d(mg, w, reads):
    b = mg.PnnxBuilder(seed=15)
    x = b.input((2, 16, 8, 16))
    p = b.silu(b.conv(x, 16, 1))                 # conv_0
    o = b.conv(x, w, 1)                          # conv_1: ODD
    dw = b.conv(p, 16, 3, groups=16)             # conv_2: si_hip_conv2d_depthwise_f16
    if reads:                                    # ... reading p at the concat's row (in_ld 20)
        b.output(b.cat([b.cat([p, o]), dw]))
        piece = p
    else:                                        # ... writing the concat's row (out_ld 20)
        b.output(b.cat([dw, o]))
        piece = dw
    return dict(b=b, shape=(2, 8, 16, 16), piece=(piece, 0, 16 + w), layers=["conv_2"],
                route=lambda k, s, prof: k["conv_2"].startswith("conv_depthwise_f16"))


def fam_e(mg, w, reads):
    b = mg.PnnxBuilder(seed=16)
    x = b.input((2, 16, 8, 16))
    p = b.silu(b.conv(x, 32, 1))                 # conv_0
    o = b.conv(x, w, 1)                          # conv_1: ODD
    s = b.hardsigmoid(b.conv(b.adaptive_avgpool(p), 32, 1))   # conv_2: the squeeze-excite scale [N, 1, 1, C]
    m = b.mul(p, s)                              # si_hip_binary_bcast_f16
    if reads:                                    # ... with the multiplicand at the concat's row
        b.output(b.cat([b.cat([p, o]), m]))
        piece = p
    else:                                        # ... writing the concat's row
        b.output(b.cat([m, o]))
        piece = "pnnx_expr_0_mul(%s,%s)" % (p, s)   # (expression lowering renames the operand on the engine side)
    binary = lambda prof: [L for L in prof if L["type"] == "BinaryOp"]
    return dict(b=b, shape=(2, 8, 16, 16), piece=(piece, 0, 32 + w), layers=None,
                route=lambda k, sc, prof: len(binary(prof)) == 1 and binary(prof)[0]["kernel"] == "binary" and
                not any(n.startswith(binary(prof)[0]["name"] + ".") for n in sc["run"]))


def fam_f(mg, w):
    b = mg.PnnxBuilder(seed=17)
    x = b.input((2, 16, 8, 16))
    t = b.conv(x, 16 + w, 1)                     # conv_0
    v, r = b.split(t, (16, w))                   # v: a view of t at t's row (AliasSplits)
    y = b.silu(b.conv(v, 32, 3))                 # conv_1: si_hip_conv2d_f16, in_ld 20
    b.output(b.cat([y, r]))
    return dict(b=b, shape=(2, 8, 16, 16), piece=(v, 0, 16 + w), layers=["conv_1"], route=lambda k, s, prof: "f16" in k["conv_1"])


def fam_g(mg, w, c=128):
    b = mg.PnnxBuilder(seed=18)
    x = b.input((2, 16, 8, 16))
    skip = b.silu(b.conv(x, c, 1))               # conv_0
    low = b.silu(b.conv(x, c, 3, 2))             # conv_1: the 4 x 8 map
    o = b.conv(x, w, 3, 2)                       # conv_2: ODD'
    y = b.silu(b.conv(b.cat([b.upsample(low, 2.0), skip]), c, 1))   # conv_3 reads `low` at the source: si_hip_conv2d_upcat_f16, up.ld 132
    z = b.upsample(b.cat([low, o]), 2.0)         # ... and `low` is the first piece of cat_1
    b.output(b.cat([y, z]))
    return dict(b=b, shape=(2, 8, 16, 16), piece=(low, 0, c + w), layers=["conv_3"],
                route=lambda k, s, prof: k["conv_3"].startswith("conv_igemm_f16_kernel<") and k["conv_3"].endswith(", true>") and
                "upsample_0" in s["fused"])


def fam_h(mg, w):
    b = mg.PnnxBuilder(seed=19)
    x = b.input((2, 16, 8, 16))
    p = b.silu(b.conv(x, 32, 1))                 # conv_0
    o = b.conv(x, w, 1)                          # conv_1: ODD
    p2 = b.silu(b.conv(x, 32, 1))                # conv_2
    g = b.cat([p, o, p2])                        # cat_0, first in the file: p lives here, at a row of 68
    m1 = b.maxpool(p, 5, 1, 2)
    m2 = b.maxpool(m1, 5, 1, 2)
    m3 = b.maxpool(m2, 5, 1, 2)                  # si_hip_maxpool5_chain3_f16 reads p there
    b.output(b.cat([g, b.cat([p, m1, m2, m3])]))
    return dict(b=b, shape=(2, 8, 16, 16), piece=(p, 0, 64 + w), layers=["maxpool_0"],
                route=lambda k, s, prof: k["maxpool_0"] == "maxpool5_chain3" and {"maxpool_1", "maxpool_2"} <= set(s["fused"]))


def fam_i(mg, w, z_piece):
    b = mg.PnnxBuilder(seed=20)
    x = b.input((2, 16, 8, 16))
    t = b.silu(b.conv(x, 64, 1))                 # conv_0: the last bottleneck's input and shortcut
    z = b.silu(b.conv(x, 64, 1))                 # conv_1: the C3's other branch
    m = b.silu(b.conv(t, 64, 1))                 # conv_2
    y = b.add(b.silu(b.conv(m, 64, 3)), t)       # conv_3
    out3 = b.silu(b.conv(b.cat([y, z]), 128, 1))  # conv_4: pair + concat + cv3 in one launch under fuse_pw = 2 (si_hip_conv2d_pw_cv3_f16)
    o = b.conv(x, w, 1)                          # conv_5: ODD
    if z_piece:                                  # ... with z at a row of 68 (z_ld)
        b.output(b.cat([b.cat([z, o]), out3]))
        piece = (z, 0, 64 + w)
    else:                                        # ... writing a row of 132
        b.output(b.cat([out3, o]))
        piece = (out3, 0, 128 + w)
    return dict(b=b, shape=(2, 8, 16, 16), piece=piece, layers=["conv_4"], opts=dict(fuse_pw=2),
                route=lambda k, s, prof: k["conv_4"] == "conv_pw_patch_f16_kernel<pw + 3x3 + cv3>" and {"conv_2", "conv_3", "cat_0"} <= set(s["fused"]))


FAMILIES = {
    "A_conv_reader": fam_a,
    "B_siblings": fam_b,
    "C1_patch_pair_c32": lambda mg, w: fam_c1(mg, w, 32, 8),
    "C1_patch_pair_c64": lambda mg, w: fam_c1(mg, w, 64, 4),
    "D_depthwise_writes": lambda mg, w: fam_d(mg, w, False),
    "D_depthwise_reads": lambda mg, w: fam_d(mg, w, True),
    "E_se_scale_writes": lambda mg, w: fam_e(mg, w, False),
    "E_se_scale_reads": lambda mg, w: fam_e(mg, w, True),
    "F_split_view": fam_f,
    "G_upsampled_source": fam_g,
    "H_pool_chain": fam_h,
    "I_cv3_output": lambda mg, w: fam_i(mg, w, False),
    "I_cv3_z": lambda mg, w: fam_i(mg, w, True),
}


def check_family(si, tmp_path, name, w, build):
    mg = si.modelgen
    case = build(mg, w)
    b, shape, opts = case["b"], case["shape"], case.get("opts", {})
    pp, bp = _save(tmp_path, b, "%s_%d" % (name, w))
    x = mg.synth_input(shape)
    # the fp64 evaluation and the fp16-storage emulation: once, shared by the assertions below (`ref_images`: of the first images only -- every
    # operator here is per-image, and the bit comparisons cover the whole batch)
    nref = case.get("ref_images", shape[0])
    exact = ref.eval_graph(b, x[:nref])
    emulated = ref.eval_graph(b, x[:nref], rnd=ref.round_f16)

    # 1. the graph is the one intended: arithmetic on the builder's shapes, and the fp32 engine's alias
    piece, offset, width = case["piece"]
    assert offset * 2 % 16 == 0, (offset,)
    assert (width % 8 != 0) == (w == ODD), (width, w)
    e32, (got32,) = _engine(si, pp, bp, x, **opts)
    assert piece in e32.schedule()["alias"], (piece, e32.schedule()["alias"])

    # 3. fp16 storage loads and runs, twice (the second forward runs on whatever a first-use path left behind)
    dense_opts = dict(opts, fp16=1, alias_cat=0, alias_split=0)
    e16, (first, second) = _engine(si, pp, bp, x, forwards=2, fp16=1, **opts)
    assert np.isfinite(first).all()

    # 2. the twin takes the route under test, with no cast pair around it
    if w == TWIN:
        k, sched, prof = _kernels(e16), e16.schedule(), e16.profile()
        assert case["route"](k, sched, prof), (k, sched["fused"], sched["run"])
        for layer in case["layers"] or []:
            assert not any(n.startswith(layer + ".in_to_f32") or n.startswith(layer + ".out_to_f16") for n in sched["run"]), sched["run"]

    # 4. bits: the same engine with every operand dense
    _, (dense,) = _engine(si, pp, bp, x, **dense_opts)
    if case.get("bits", True):
        assert_exact(_bits(first), _bits(dense), name + ": fp16 on views vs every operand dense")
        assert_exact(_bits(second), _bits(dense), name + ": the second forward")
        _, replays = _engine(si, pp, bp, x, forwards=4, fp16=1, graph=1, **opts)
        for i, r in enumerate(replays):
            assert_exact(_bits(r), _bits(dense), name + ": graph=1, forward %d" % i)
        _, (noarena,) = _engine(si, pp, bp, x, fp16=1, arena=0, **opts)
        assert_exact(_bits(noarena), _bits(dense), name + ": arena=0")
        _, (unfused,) = _engine(si, pp, bp, x, fp16=1, fuse=0, **opts)
        _, (unfused_dense,) = _engine(si, pp, bp, x, fuse=0, **dense_opts)
        assert_exact(_bits(unfused), _bits(unfused_dense), name + ": fuse=0, on views vs dense")
    if w == ODD:   # no more cast steps than the twin's plan has (a silent detour through fp32 is not a fix)
        twin = si.Engine(fp16=1, **opts)
        twin.load_model(*_save(tmp_path, build(mg, TWIN)["b"], "%s_twin_plan" % name))
        assert len(_casts(e16)) <= len(_casts(twin)), (_casts(e16), _casts(twin))

    # 5. values: against fp64 at most 2x the error of the fp16-storage emulation (the factor of test_toy_fp16_storage)
    e_engine, e_emu = util.rel_err(first[:nref], exact), util.rel_err(emulated, exact)
    print("%s w=%d fp16 storage vs fp64: engine %.3e, fp16 emulation %.3e" % (name, w, e_engine, e_emu))
    assert e_engine <= 2.0 * e_emu, (e_engine, e_emu)

    # 6. the fp32 control: the default engine against its plain schedule, at the bar of test_graph_parity_vs_oracle -- and against fp64
    _, (plain32,) = _engine(si, pp, bp, x, fuse=0, alias_cat=0, **opts)
    assert_parity(got32, plain32, 1e-6, what=name + " fp32 fused vs unfused")
    assert_parity(got32[:nref], exact, what=name + " fp32 vs fp64")
    return e16


@pytest.mark.parametrize("w", [ODD, TWIN], ids=["odd", "twin"])
@pytest.mark.parametrize("name", sorted(FAMILIES))
def test_fp16_storage_on_a_view_the_kernel_refuses(si, tmp_path, name, w):
    """One family of the module docstring, ODD or TWIN.  Before the planner asked (read from the code, not run): A, B, C1, D, E, F, G and I_cv3_z
    loaded and failed at the first Forward with kUnsupport; H (the three-pool fallback) and I_cv3_output (2-byte stores at any row) were fine."""
    check_family(si, tmp_path, name, w, FAMILIES[name])


@pytest.mark.parametrize("w", [ODD, TWIN], ids=["odd", "twin"])
def test_slab_pair_writing_an_odd_row_runs_as_two_launches(si, tmp_path, w):
    """C2: the 128-channel bottleneck pair at 40 x 40, batch 32 (the shape test_bottleneck_pairs_in_one_launch_with_fp16_storage shows fused in the
    slab kernel) writing the first piece of a 132-wide concat.  The slab form refuses out_ld 132 and the layer runs its two launches through a
    private intermediate -- device memory: until this change a default-constructed (host) Tensor, so the 1x1 conv was handed pageable host
    memory as its destination.  The planner keeps the alias: the two launches take any output row."""
    e16 = check_family(si, tmp_path, "C2_slab_pair", w, fam_c2)
    q = fam_c2(si.modelgen, w)["piece"][0]
    assert q in e16.schedule()["alias"], e16.schedule()["alias"]    # the fp16 engine keeps the view: the fallback is what serves it


def _f32_rows(mg, which):
    """B and G with rows that fp32 kernels refuse (3 extra channels: 515 and 131 floats) and layers wide enough for f32_split to take"""
    if which == "B":
        case = fam_b(mg, 3, 256, 128, 128)
        case["layer"] = "conv_2"
        return case
    case = fam_g(mg, 3, 128)
    case["layer"] = "conv_3"
    return case


@pytest.mark.parametrize("which", ["B", "G"])
def test_f32_split_on_a_row_the_split_kernels_refuse(si, tmp_path, which):
    """fp32 storage, f32_split = 1.  B: the sibling-fused 1x1 pair reads p at a row of 515 floats; si_hip_conv2d_split3_split_f32 refuses it, the
    layer is demoted and the result is the default engine's, bit for bit.  G: `low` would sit at a row of 131 floats as the first piece of a
    concat while the dual-source conv reads it at the source; neither si_hip_conv2d_split3_upcat_f32 nor the fp32 kernel behind a demotion
    takes that row, so the planner declines the alias in fp32 as well and the layer stays on the split kernel, at the f32_split parity bar."""
    mg = si.modelgen
    case = _f32_rows(mg, which)
    b, shape = case["b"], case["shape"]
    pp, bp = _save(tmp_path, b, "f32rows_" + which)
    x = mg.synth_input(shape)
    exact = ref.eval_graph(b, x)
    e0, (want,) = _engine(si, pp, bp, x)
    assert_parity(want, exact, what=which + " fp32 vs fp64")
    _, (plain,) = _engine(si, pp, bp, x, fuse=0, alias_cat=0)
    assert_parity(want, plain, 1e-6, what=which + " fp32 fused vs unfused")
    piece, _, width = case["piece"]
    assert width % 4 != 0
    e1, (got, again) = _engine(si, pp, bp, x, forwards=2, f32_split=1)
    sch = e1.schedule()
    k0, k1 = _kernels(e0)[case["layer"]], _kernels(e1)[case["layer"]]
    print("%s: default [%s], f32_split [%s], split_demoted %s, alias %s" % (which, k0, k1, sch["split_demoted"], sch["alias"]))
    if which == "B":
        assert piece in sch["alias"] and "conv_3" in sch["fused"]
        assert sch["split_demoted"] == [case["layer"]] and sch["split_reruns"] == 0, sch
        assert_exact(_bits(got), _bits(want), "B: f32_split on a refused row vs the default engine")
        assert_exact(_bits(again), _bits(want), "B: the second forward, on the re-packed weights")
    else:
        assert "upsample_0" in sch["fused"] and piece not in sch["alias"] and piece not in e0.schedule()["alias"], sch
        assert "split3" in k1 and sch["split_demoted"] == [], (k1, sch)
        assert_parity(got, exact, what="G: f32_split on the dual-source layer vs fp64")    # (tests/test_gpu_engine.py: f32_split holds the fp32 bars)
        assert_exact(_bits(again), _bits(got), "G: the second forward")


def test_a_graph_fp16_cannot_serve_fails_at_load(si, tmp_path):
    """The other half of the promise: what fp16 storage really cannot serve -- an LSTM over 20 hidden units between half tensors, which has neither
    an fp16 step kernel nor an fp32 form between casts -- is a status from load_model, with nothing left for the first Forward to find; the
    same file loads and runs without the option."""
    mg = si.modelgen
    b = mg.PnnxBuilder(seed=3)
    b.output(b.relu(b.lstm(b.relu(b.input((7, 2, 8))), 20)))
    pp, bp = _save(tmp_path, b, "h20")
    e = si.Engine(fp16=1)
    with pytest.raises(si.StatusError) as ei:
        e.load_model(pp, bp)
    assert ei.value.status == si.Status.kUnsupport, ei.value.status
    e32 = si.Engine()
    e32.load_model(pp, bp)
    e32.input(e32.input_names()[0], mg.synth_input((7, 2, 8)))
    e32.forward()
    assert np.isfinite(e32.extract(e32.output_names()[0])).all()
