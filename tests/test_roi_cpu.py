"""CPU: torchvision.ops.RoIAlign / roi_align without a device.  The numpy restatement (tests/roi_reference.py) against hand-computed values, the
`aligned` half-pixel shift, the builders' lines and both toys, the registry, include/si_roi.h against _native.py, the refusals of the entries
(before any device call), the kernel-name predicate, and two stand-alone C++ programs under AddressSanitizer and UBSan: the batch rule for
both type strings (tests/cpp/test_roi_rule.cpp) and the termination arithmetic the kernel shares with the host
(tests/cpp/test_roi_interval.cpp over csrc/hip/roi_interval.h), where the extreme boxes are tried."""
import ctypes as C
import os
import re
import subprocess
import time

import numpy as np

import containment as ct
import roi_reference as rr
import util
from ct_reference import _parse
from simpleinfer_amd import _native, engine, hipops, modelgen as mg

BADARG, UNSUPPORTED = -1, -2


# ---- the restatement --------------------------------------------------------------------------------------------------------
def test_one_bin_over_a_constant_map():
    x = np.full((1, 6, 7, 3), 2.5, np.float32)
    for ratio in (-1, 1, 2, 5):
        for aligned in (False, True):
            y = rr.roi_align_ref(x, [[0, 1.0, 1.0, 5.0, 4.0]], 1, 1.0, ratio, aligned)
            assert y.shape == (1, 1, 1, 3) and np.array_equal(y, np.full((1, 1, 1, 3), 2.5)), (ratio, aligned, y)


def test_samples_on_exact_pixel_centres():
    """scale 1, aligned=False, the box [1, 2, 5, 6] pooled 2 x 2 with one sample per bin: bins 2 x 2 px, samples at (3, 2), (3, 4), (5, 2), (5, 4)
    (y, x): each output is that pixel.  With two samples per axis they fall on y = 2.5, 3.5, .. : the mean of the four pixels round them."""
    x = np.arange(8 * 9, dtype=np.float32).reshape(1, 8, 9, 1)
    y = rr.roi_align_ref(x, [[0, 1.0, 2.0, 5.0, 6.0]], 2, 1.0, 1, False)[0, :, :, 0]
    assert np.array_equal(y, [[x[0, 3, 2, 0], x[0, 3, 4, 0]], [x[0, 5, 2, 0], x[0, 5, 4, 0]]])
    y2 = rr.roi_align_ref(x, [[0, 1.0, 2.0, 5.0, 6.0]], 2, 1.0, 2, False)[0, :, :, 0]
    # samples of bin (0, 0): y in {2.5, 3.5}, x in {1.5, 2.5}: a linear ramp, so the mean is the ramp at (3, 2)
    assert np.array_equal(y2, y)
    # adaptive: ceil(4 / 2) = 2 samples per axis, the same
    assert np.array_equal(rr.roi_align_ref(x, [[0, 1.0, 2.0, 5.0, 6.0]], 2, 1.0, 0, False)[0, :, :, 0], y)


def test_a_box_wholly_outside_is_zero_and_the_borders_are_sharp():
    x = util.rng_uniform(1, (2, 5, 6, 4), 0.5, 1.5)
    assert np.array_equal(rr.roi_align_ref(x, [[1, 20.0, 20.0, 30.0, 30.0], [0, -30.0, 2.0, -20.0, 4.0]], (2, 3), 1.0, 2, False), np.zeros((2, 2, 3, 4)))
    # one sample exactly at y = -1 and at y = h is inside (clamped to the border row), one ulp beyond is not
    col = np.arange(5, dtype=np.float32).reshape(1, 5, 1, 1) + 1.0
    at = lambda yc: rr.roi_align_ref(col, [[0, 0.0, yc - 0.5, 1.0, yc + 0.5]], 1, 1.0, 1, False)[0, 0, 0, 0]
    assert at(-1.0) == 1.0 and at(5.0) == 5.0 and at(0.0) == 1.0 and at(4.0) == 5.0 and at(3.5) == 4.5
    assert at(np.float32(-1.5)) == 0.0 and at(np.float32(5.5)) == 0.0
    # zero size: without `aligned` the box is widened to 1 px, with it the bin is empty but the sample stays (count 1)
    one = rr.roi_align_ref(col, [[0, 0.0, 2.0, 0.0, 2.0]], 1, 1.0, 1, False)[0, 0, 0, 0]
    assert one == 3.5
    assert rr.roi_align_ref(col, [[0, 0.0, 2.0, 0.0, 2.0]], 1, 1.0, 1, True)[0, 0, 0, 0] == 2.5


def test_aligned_shifts_by_half_a_pixel():
    """aligned=True at scale s samples where aligned=False samples the box moved by -0.5 / s -- for boxes at least a pixel wide, where the
    fmaxf(.., 1) of the unaligned form does nothing"""
    x = util.rng_uniform(2, (1, 9, 11, 2), -1.0, 1.0)
    for scale in (1.0, 0.25):
        box = np.asarray([0, 2.0, 1.0, 7.0, 6.0], np.float32)
        box[1:] /= scale
        moved = box.copy()
        moved[1:] -= 0.5 / scale
        a = rr.roi_align_ref(x, [box], (3, 2), scale, 2, True)
        b = rr.roi_align_ref(x, [moved], (3, 2), scale, 2, False)
        assert np.array_equal(a, b), scale
        assert not np.array_equal(a, rr.roi_align_ref(x, [box], (3, 2), scale, 2, False))


def test_invalid_boxes_are_nan_rows():
    x = util.rng_uniform(3, (2, 5, 6, 3), -1.0, 1.0)
    good = [0, 1.0, 1.0, 4.0, 3.0]
    bad = [[-1, 1, 1, 4, 3], [2, 1, 1, 4, 3], [0.5, 1, 1, 4, 3], [np.nan, 1, 1, 4, 3], [0, np.nan, 1, 4, 3], [1, 1, np.inf, 4, 3], [0, 1, 1, -np.inf, 3],
           [0, 0, 0, 1e9, 1e9]]
    y = rr.roi_align_ref(x, [good] + bad + [good], 2, 1.0, 0, False)
    assert np.isnan(y[1:-1]).all() and np.isfinite(y[0]).all() and np.array_equal(y[0], y[-1])
    assert np.isfinite(rr.roi_align_ref(x, [[0, 0, 0, 1e9, 1e9]], 2, 1.0, 2, False)).all()      # fixed sampling: two samples, wherever they fall


def test_the_reference_runs_the_whole_matrix_in_seconds():
    """a cap, not a measurement: every combination of the GPU matrix, 70 boxes and 16 channels each, the 4096 px box included"""
    rr._MATRIX_REF.clear()
    t0 = time.perf_counter()
    for p in rr.matrix_params():
        ref = rr.matrix_ref(*p)
        assert ref.shape == (70,) + p[0] + (16,) and np.isfinite(ref).all()
    took = time.perf_counter() - t0
    print("reference over %d combinations: %.2f s" % (len(rr.matrix_params()), took))
    assert len(rr.matrix_params()) == 90 and took < 20.0, took
    # the hand-made boxes do what their comments say, at every scale
    for scale in rr.MATRIX_SCALE:
        rois = rr.matrix_rois(scale)
        assert rois.shape == (70, 5) and rois.dtype == np.float32 and set(rois[:, 0]) == {0.0, 1.0}
        assert np.array_equal(rois[:, 1:] * np.float32(scale), rr.matrix_rois(1.0)[:, 1:])          # exact: powers of two
        assert (rois[10, 3] - rois[10, 1]) * scale == 4096.0
    ref = rr.matrix_ref((2, 3), 2, False, 1.0)
    assert not ref[5].any() and not ref[6].any() and ref[0].any()
    # the 4096 px box: two samples per bin all fall outside the map, the adaptive 1366 per bin reach it
    assert not ref[10].any() and rr.matrix_ref((2, 3), 0, False, 1.0)[10].any()


# ---- builders ---------------------------------------------------------------------------------------------------------------
def _types(b):
    return [_parse(ln)[0] for ln in b.lines]


def test_builder_lines_parse_back():
    b = mg.PnnxBuilder(seed=1)
    x, r = b.input((2, 6, 9, 11)), b.input((7, 5))
    y = b.roi_align(x, r, (3, 4), 0.25, 2, True)
    p = _parse(b.lines[-1])
    assert b.lines[-1].split()[:7] == ["torchvision.ops.RoIAlign", "roialign_0", "2", "1", x, r, y]
    assert p[4] == dict(aligned="True", output_size="(3,4)", sampling_ratio="2", spatial_scale="2.500000e-01") and b.shapes[y] == (7, 6, 3, 4)
    assert b.lines[-1].endswith("#0=(2,6,9,11)f32 #1=(7,5)f32 #2=(7,6,3,4)f32")
    y2 = b.roi_align(x, r, 7, functional=True)
    p = _parse(b.lines[-1])
    assert p[0] == "torchvision.ops.roi_align" and p[1] == "torchvision_ops_roi_align_0" and b.shapes[y2] == (7, 6, 7, 7)
    assert p[4] == dict(aligned="False", output_size="(7,7)", sampling_ratio="-1", spatial_scale="1.000000e+00")


def test_toys_have_the_expected_operator_sequence():
    b = mg.build_toy_box_head()
    assert _types(b) == ["pnnx.Input", "pnnx.Input", rr.TYPES[0], "nn.Conv2d", "nn.ReLU", "torch.flatten", "nn.Linear", "nn.ReLU", "nn.Linear", "nn.Linear",
                         "pnnx.Output", "pnnx.Output"]
    lines = [_parse(ln) for ln in b.lines]
    pool = lines[2]
    assert pool[2] == [lines[0][3][0], lines[1][3][0]] and pool[4] == dict(aligned="False", output_size="(7,7)", sampling_ratio="2", spatial_scale="2.500000e-01")
    assert b.shapes[pool[3][0]] == (6, 8, 7, 7) and b.shapes[lines[5][3][0]] == (6, 16 * 49)
    assert [b.shapes[ln[2][0]] for ln in lines[-2:]] == [(6, 5), (6, 20)] and lines[8][2] == lines[9][2] == lines[7][3]
    m = mg.build_toy_mask_head()
    assert _types(m) == ["pnnx.Input", "pnnx.Input", rr.TYPES[1], "nn.Conv2d", "nn.ReLU", "nn.Conv2d", "nn.ReLU", "nn.ConvTranspose2d", "nn.ReLU", "nn.Conv2d",
                         "nn.Sigmoid", "pnnx.Output"]
    lines = [_parse(ln) for ln in m.lines]
    assert lines[2][4] == dict(aligned="True", output_size="(14,14)", sampling_ratio="2", spatial_scale="2.500000e-01")
    assert lines[7][4]["kernel_size"] == "(2,2)" and lines[7][4]["stride"] == "(2,2)" and lines[9][4]["kernel_size"] == "(1,1)"
    assert m.shapes[lines[2][3][0]] == (5, 8, 14, 14) and m.shapes[lines[-1][2][0]] == (5, 3, 28, 28)
    assert mg.build_toy_box_head(batch=3, boxes=9).shapes["1"] == (9, 5)
    r = mg.toy_rois(6, 2, 20, 24)
    assert r.shape == (6, 5) and r.dtype == np.float32 and list(r[:, 0]) == [0, 1, 0, 1, 0, 1] and (r[:, 3] > r[:, 1]).all() and (r[:, 4] > r[:, 2]).all()


def test_toys_evaluate_with_torch_around_the_reference():
    b = mg.build_toy_box_head()
    feat, rois = mg.synth_input((2, 20, 24, 8)), mg.toy_rois(6, 2, 20, 24)
    scores, deltas = rr.eval_graph(b, [feat, rois])
    assert scores.shape == (6, 5) and deltas.shape == (6, 20) and np.isfinite(scores).all() and np.isfinite(deltas).all()
    sh, _ = rr.eval_graph(b, [feat, rois], rnd=rr.round_f16)
    assert 0.0 < np.abs(sh - scores).max() < 5e-2 * np.abs(scores).max()
    # rows are independent: permuting the boxes permutes the rows
    perm = np.asarray([3, 0, 5, 1, 4, 2])
    s2, _ = rr.eval_graph(b, [feat, rois[perm]])
    assert np.allclose(s2, scores[perm], rtol=0, atol=1e-12)
    m = mg.build_toy_mask_head()
    (masks,) = rr.eval_graph(m, [feat, mg.toy_rois(5, 2, 20, 24)])
    assert masks.shape == (5, 28, 28, 3) and (masks > 0).all() and (masks < 1).all()


# ---- registry and batch rule ------------------------------------------------------------------------------------------------
def test_registry_lists_both_types(native_libs):
    assert set(rr.TYPES) <= set(engine.registry_types())


SANITIZE = ["-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"]      # the runtimes inside the program: it starts the same under any environment


def test_batch_rule_for_both_types_stand_alone_under_sanitizers(tmp_path):
    host = os.path.join(rr.ROOT, "simpleinfer_amd", "csrc", "host")
    exe = str(tmp_path / "test_roi_rule")
    subprocess.check_call(["g++", "-std=c++17", "-O0", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined"] + SANITIZE +
                          ["-I" + host, os.path.join(rr.ROOT, "tests", "cpp", "test_roi_rule.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "roi rule ok" in r.stdout, r.stdout[-4000:] + r.stderr[-4000:]


def test_termination_arithmetic_stand_alone_under_sanitizers(tmp_path):
    """the header the kernel includes, compiled for the host: the interval holds every inside sample (brute force), the trip count is bounded,
    no float -> int conversion overflows (UBSan's float-cast check), NaN / Inf / a bad image index are invalid"""
    exe = str(tmp_path / "test_roi_interval")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-ffp-contract=off", "-fsanitize=address,undefined,float-cast-overflow"] +
                          SANITIZE + ["-I" + os.path.dirname(rr.INTERVAL_HEADER), os.path.join(rr.ROOT, "tests", "cpp", "test_roi_interval.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "roi interval ok" in r.stdout and "runtime error" not in r.stderr, r.stdout[-4000:] + r.stderr[-4000:]
    # the numbers the documents quote are the header's
    text = open(rr.INTERVAL_HEADER).read()
    assert "#define SI_ROI_GRID_LIMIT %d " % rr.GRID_LIMIT in text and "#define SI_ROI_RATIO_LIMIT 256" in text
    assert "#define SI_ROI_TRIP_BOUND(size) (2 * (size) + 8)" in text
    assert '#include "roi_interval.h"' in open(os.path.join(os.path.dirname(rr.INTERVAL_HEADER), "roi_align.hip")).read()


def test_the_restatement_decides_as_the_header_does():
    """roi_setup of the restatement against the extreme values of the C++ program (the same verdicts)"""
    v = lambda roi, scale=1.0, ratio=0, aligned=False: rr.roi_setup(roi, 2, 7, 7, scale, ratio, aligned) is not None
    assert v([0, 0, 0, 0, 0]) and v([1, 1, 1, 2, 2]) and v([0, 0, 0, 1e30, 1e30], ratio=2)
    assert not v([0, 0, 0, 1e9, 1e9]) and not v([0, 0, 0, 1e30, 1e30]) and not v([0, -3e38, 0, 3e38, 1], ratio=2) and not v([0, 0, 0, 3e38, 1], 16.0, 2)
    assert not v([2, 1, 1, 2, 2]) and not v([0.5, 1, 1, 2, 2]) and not v([np.nan, 1, 1, 2, 2]) and not v([0, 1, np.inf, 2, 2])
    assert rr.roi_setup([0, 0, 0, 7 * 4194304.0, 7.0], 1, 7, 7, 1.0, 0, False)[5] == 4194304          # exactly the limit is served


# ---- C-ABI ------------------------------------------------------------------------------------------------------------------
def _declared(path):
    src = open(path).read()
    src = re.sub(r"/\*.*?\*/", " ", src, flags=re.S)
    src = re.sub(r"//[^\n]*", " ", src)
    names = []
    for m in re.finditer(r"\b(si_[a-z0-9_]+)\s*\(", src):
        if m.group(1) not in names:
            names.append(m.group(1))
    return names


def test_roi_header_is_exported_and_bound(native_libs):
    H, _ = native_libs
    declared = _declared(rr.HEADER)
    assert sorted(declared) == sorted(rr.ENTRIES)
    assert sorted(H._si_roi_signatures) == sorted(declared)
    for other in (H._si_signatures, H._si_norm_signatures, H._si_pad_signatures, H._si_pool_signatures, H._si_softmax_signatures, H._si_permute_signatures,
                  H._si_attention_signatures, H._si_deform_signatures, H._si_grid_signatures):
        assert not set(declared) & set(other)
    raw = C.CDLL(_native.LIB_HIP_PATH)   # a handle of its own: nothing but the dynamic symbol table answers
    missing = [name for name in declared if not hasattr(raw, name)]
    assert not missing, missing
    # the Python structure has the header's fields in the header's order, with the header's types
    ctypes_of = {"int": C.c_int, "float": C.c_float}
    m = re.search(r"typedef struct SiRoiAlignDesc \{(.*?)\} SiRoiAlignDesc;", open(rr.HEADER).read(), flags=re.S)
    body = re.sub(r"/\*.*?\*/", " ", m.group(1), flags=re.S)
    fields = [(n.strip(), ctypes_of[typ]) for typ, names in re.findall(r"\b(int|float)\s+([^;]+);", body) for n in names.split(",")]
    assert fields == list(_native.SiRoiAlignDesc._fields_), fields
    assert C.sizeof(_native.SiRoiAlignDesc) == 13 * 4
    text = open(ct.HEADER).read()
    assert "SiRoiAlignDesc" not in text and "roi_align" not in text


def _desc(**kw):
    args = dict(x_shape=(2, 9, 11, 8), k=6, output_size=(7, 7), sampling_ratio=2)
    args.update(kw)
    return hipops.roi_align_desc(**args)


def test_refusals_without_a_device(native_libs):
    """refusals happen before any device call: the launch entries return the code, the name entry "none" """
    H, _ = native_libs
    P = [C.c_void_p((j + 1) << 28) for j in range(3)]   # x, rois, out: 256 MiB apart

    def check(d, code, p=P, what=""):
        ref = C.byref(d) if d is not None else None
        for half, fn in ((0, H.si_hip_roi_align_f32), (1, H.si_hip_roi_align_f16)):
            got = fn(ref, p[0], p[1], p[2], None)
            assert got == code, (what, half, got)
            assert H.si_hip_roi_align_kernel_name(ref, p[0], p[1], p[2], half) == b"none", (what, half)

    check(None, BADARG, what="null descriptor")
    assert H.si_hip_roi_align_kernel_name(C.byref(_desc()), P[0], P[1], P[2], 0) == b"roi_align_kernel<float, 4>"
    for j in range(3):
        check(_desc(), BADARG, [None if i == j else P[i] for i in range(3)], "null pointer %d" % j)
    for field in ("n", "c", "h", "w", "k", "ph", "pw"):
        for value in (0, -1):
            bad = _desc()
            setattr(bad, field, value)
            check(bad, BADARG, what=(field, value))
    for field, value in (("in_ld", 7), ("out_ld", 7), ("in_ld", -8), ("rois_ld", 4), ("rois_ld", -5)):
        bad = _desc()
        setattr(bad, field, value)
        check(bad, BADARG, what=(field, value))
    # the output's extent intersecting x or the boxes
    check(_desc(), BADARG, [P[0], P[1], P[0]], "out == x")
    check(_desc(), BADARG, [P[0], P[1], C.c_void_p(P[0].value + 64)], "out inside x")
    check(_desc(), BADARG, [P[0], P[1], C.c_void_p(P[0].value - 64)], "x inside out")
    check(_desc(), BADARG, [P[0], P[1], P[1]], "out == rois")
    check(_desc(), BADARG, [P[0], P[1], C.c_void_p(P[1].value + 4 * 29)], "out begins at the last float of the boxes")
    check(_desc(rois_ld=8), BADARG, [P[0], P[1], C.c_void_p(P[1].value + 4 * 44)], "... with a row stride")
    ok = [P[0], P[1], C.c_void_p(P[1].value + 4 * 30)]                    # the output starts where the boxes end
    assert H.si_hip_roi_align_kernel_name(C.byref(_desc()), ok[0], ok[1], ok[2], 0) == b"roi_align_kernel<float, 1>"       # (and is 8-byte aligned only)
    ok = [P[0], P[1], C.c_void_p(P[1].value - 6 * 49 * 8 * 2)]            # the fp16 output ends where the boxes start
    assert H.si_hip_roi_align_kernel_name(C.byref(_desc()), ok[0], ok[1], ok[2], 1) != b"none"
    check(_desc(), BADARG, [P[0], P[1], C.c_void_p(P[1].value - 6 * 49 * 8 * 2 + 2)], "the boxes' first byte is the fp16 output's last")
    # beyond the limits: a sampling_ratio above 256, element offsets beyond 31 bits, sizes beyond 2^24 (they are used as floats)
    far = [C.c_void_p((j + 1) << 44) for j in range(3)]
    check(_desc(sampling_ratio=257), UNSUPPORTED, far, "sampling_ratio")
    assert H.si_hip_roi_align_kernel_name(C.byref(_desc(sampling_ratio=256)), far[0], far[1], far[2], 0) != b"none"
    for ratio in (0, -1, -7):
        assert H.si_hip_roi_align_kernel_name(C.byref(_desc(sampling_ratio=ratio)), far[0], far[1], far[2], 0) != b"none"
    for field, value in (("in_ld", 1 << 30), ("out_ld", 1 << 30), ("rois_ld", 1 << 30)):
        bad = _desc()
        setattr(bad, field, value)
        check(bad, UNSUPPORTED, far, what=field)
    check(hipops.roi_align_desc((1 << 15, 256, 256, 1), 1, 1), UNSUPPORTED, far, "2^31 input pixels")
    check(hipops.roi_align_desc((1, 4, 4, 1), 1 << 15, (256, 256)), UNSUPPORTED, far, "2^31 output bins")
    check(hipops.roi_align_desc((1, 1, (1 << 24) + 1, 1), 1, 1), UNSUPPORTED, far, "w beyond 2^24")
    assert H.si_hip_roi_align_kernel_name(C.byref(hipops.roi_align_desc((1, 1, 1 << 24, 1), 1, 1)), far[0], far[1], far[2], 0) != b"none"


def test_kernel_name_by_channels_strides_alignment_and_type(native_libs):
    name = hipops.roi_align_kernel_name
    xs = lambda c: (2, 9, 11, c)
    for half in (False, True):
        for c in (1, 2, 3, 4, 5, 6, 8, 12, 16, 20):
            assert name(xs(c), 5, 7, half) == rr.expected_kernel(c, half), (half, c)
    f32, f16 = (lambda vw: "roi_align_kernel<float, %d>" % vw), (lambda vw: "roi_align_kernel<_Float16, %d>" % vw)
    assert name(xs(8), 5, 7, in_ld=12, out_ld=16) == f32(4) and name(xs(8), 5, 7, in_ld=10) == f32(1) and name(xs(8), 5, 7, out_ld=9) == f32(1)
    assert [name(xs(8), 5, 7, True, in_ld=ld) for ld in (16, 12, 10, 9)] == [f16(8), f16(4), f16(2), f16(1)]
    assert [name(xs(8), 5, 7, True, out_ld=ld) for ld in (24, 20, 18, 11)] == [f16(8), f16(4), f16(2), f16(1)]
    assert [name(xs(8), 5, 7, align=a) for a in (16, 8, 4)] == [f32(4), f32(1), f32(1)]
    assert [name(xs(8), 5, 7, True, align=a) for a in (16, 8, 4, 2)] == [f16(8), f16(4), f16(2), f16(1)]
    assert name(xs(8), 5, 7, rois_ld=7) == f32(4)                      # (the boxes have no alignment rule beyond their own 4 bytes)


def test_every_compute_entry_of_the_roi_header_is_driven():
    """the rule of tests/test_containment_cpu.py for include/si_hip.h, applied to include/si_roi.h and the view cases of the GPU file"""
    import test_gpu_roi as tg
    entries = [n for n in ct.header_functions(rr.HEADER) if not ct.is_exempt(n)]
    assert sorted(entries) == ["si_hip_roi_align_f16", "si_hip_roi_align_f32"]
    driven = {c.entry for c in tg.VIEW_CASES}
    assert set(entries) <= driven and driven <= set(ct.header_functions(rr.HEADER))
