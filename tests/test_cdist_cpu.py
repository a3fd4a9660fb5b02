"""CPU: torch.cdist -- the float64 rule pinned to torch float64, the builder's lines and the two toys, the registry, the C-ABI of
include/si_cdist.h (names, structure, refusals, kernel choice) without a device, and cdist_plan.h with the kCdist batch rule as a
stand-alone C++ program under ASan and UBSan (a child process)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import cdist_reference as cr
import containment as ct
from ct_reference import _parse
from simpleinfer_amd import _native, engine, hipops, modelgen as mg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "si_cdist.h")
BADARG, UNSUPPORTED = -1, -2
INF = float("inf")


@pytest.mark.parametrize("p", [1.0, 2.0, INF])
@pytest.mark.parametrize("s1,s2", [((5, 7), (4, 7)), ((3, 5, 7), (3, 4, 7)), ((1, 5, 7), (3, 4, 7)), ((3, 5, 7), (1, 4, 7)), ((3, 5, 7), (4, 7))],
                         ids=["rank2", "rank3", "b1=1", "b2=1", "rank3-rank2"])
def test_rule_is_torch_float64(s1, s2, p):
    r = np.random.RandomState(3)
    a, b = r.standard_normal(s1), r.standard_normal(s2)
    want = torch.cdist(torch.from_numpy(a), torch.from_numpy(b), p=p, compute_mode="donot_use_mm_for_euclid_dist").numpy()
    assert np.abs(cr.cdist_ref(a, b, p) - want).max() <= 1e-12


def test_builder_lines_and_the_toys():
    b = mg.PnnxBuilder(seed=1)
    x = b.input((2, 9, 16))
    b.output(b.cdist(b.cdist(x, x), b.attribute(np.ones((5, 9))), INF, "use_mm_for_euclid_dist"))
    ops = [_parse(ln) for ln in b.lines]
    assert [o[0] for o in ops] == ["pnnx.Input", "torch.cdist", "pnnx.Attribute", "torch.cdist", "pnnx.Output"]
    assert ops[1][2] == [x, x] and ops[1][4] == {"compute_mode": "None", "p": "2.000000e+00"} and b.shapes[ops[1][3][0]] == (2, 9, 9)
    assert ops[3][4] == {"compute_mode": "use_mm_for_euclid_dist", "p": "inf"} and b.shapes[ops[3][3][0]] == (2, 9, 5)
    seq = lambda toy: [_parse(ln)[0] for ln in toy.lines]
    trunk = ["nn.Conv2d", "nn.ReLU", "nn.Conv2d", "F.normalize", "Tensor.permute", "Tensor.view"]
    toy = mg.build_toy_descriptor_matcher(2, 16, 32)
    assert seq(toy) == ["pnnx.Input", "pnnx.Input"] + trunk * 2 + ["torch.cdist", "pnnx.Output"]
    assert toy.shapes[_parse(toy.lines[-1])[2][0]] == (2, 64, 64)
    convs = [_parse(ln)[1] for ln in toy.lines if ln.startswith("nn.Conv2d")]
    assert all(np.array_equal(toy.attrs[convs[i] + ".weight"], toy.attrs[convs[i + 2] + ".weight"]) for i in (0, 1))     # one trunk, written twice
    toy = mg.build_toy_vq_encoder(2, 8, 16, 40)
    assert seq(toy) == ["pnnx.Input", "nn.Conv2d", "Tensor.permute", "Tensor.view", "pnnx.Attribute", "torch.cdist", "pnnx.Output"]
    assert toy.shapes[_parse(toy.lines[-1])[2][0]] == (2, 64, 40) and toy.attrs["pnnx_attr_0.data"].shape == (40, 16)


def test_registry_header_and_bound_table(native_libs):
    H, _ = native_libs
    types = engine.registry_types()
    assert "torch.cdist" in types and not {"F.pairwise_distance", "F.cosine_similarity", "torch.matmul", "torch.bmm"} & set(types)
    declared = ct.header_functions(HEADER)
    assert sorted(declared) == sorted(H._si_cdist_signatures) == ["si_hip_cdist_f16", "si_hip_cdist_f32", "si_hip_cdist_kernel_name"]
    others = [getattr(H, k) for k in vars(H) if k.startswith("_si_") and k.endswith("signatures") and k != "_si_cdist_signatures"]
    assert len(others) >= 20 and not any(set(declared) & set(o) for o in others)
    raw = C.CDLL(_native.LIB_HIP_PATH)   # a handle of its own: nothing but the dynamic symbol table answers
    assert all(hasattr(raw, name) for name in declared)
    m = re.search(r"typedef struct SiCdistDesc \{(.*?)\} SiCdistDesc;", open(HEADER).read(), flags=re.S)
    body = re.sub(r"/\*.*?\*/", " ", m.group(1), flags=re.S)
    fields = [(n.strip(), C.c_int) for names in re.findall(r"\bint\s+([^;]+);", body) for n in names.split(",")]
    assert fields == list(_native.SiCdistDesc._fields_) and C.sizeof(_native.SiCdistDesc) == 13 * 4


@pytest.mark.parametrize("fn,esize", [("si_hip_cdist_f32", 4), ("si_hip_cdist_f16", 2)])
def test_refusals_without_a_device(native_libs, fn, esize):
    """every refusal happens before any device call: the pointers are compared, never followed"""
    H, _ = native_libs
    a, b, o = C.c_void_p(1 << 40), C.c_void_p(1 << 41), C.c_void_p(1 << 42)
    desc = hipops.cdist_desc
    call = lambda d, x1=a, x2=b, out=o: getattr(H, fn)(C.byref(d), x1, x2, out, None)
    assert getattr(H, fn)(None, a, b, o, None) == BADARG
    named = lambda d, out: H.si_hip_cdist_kernel_name(C.byref(d), a, b, out, esize == 2).decode()
    assert named(desc((3, 5, 8), (3, 4, 8)), o) != "none"     # (the good descriptor the rest are made from; it is never launched here)
    for null in ("x1", "x2", "out"):
        assert call(desc((3, 5, 8), (3, 4, 8)), **{null: None}) == BADARG
    for field in ("b1", "b2", "p", "r", "m"):
        for value in (0, -3):
            bad = desc((3, 5, 8), (3, 4, 8))
            setattr(bad, field, value)
            assert call(bad) == BADARG, (field, value)
    assert call(desc((3, 5, 8), (2, 4, 8))) == BADARG                                                      # batches 3 and 2
    assert call(desc((5, 8), (4, 8), x1_ld=7)) == BADARG and call(desc((5, 8), (4, 8), x2_ld=7)) == BADARG and call(desc((5, 8), (4, 8), out_ld=3)) == BADARG
    bad = desc((3, 5, 8), (3, 4, 8))
    bad.x1_sb = 39
    assert call(bad) == BADARG                                                                             # batch items that meet
    assert call(desc((5, 8), (4, 8)), out=a) == BADARG and call(desc((5, 8), (4, 8)), out=C.c_void_p(b.value + 31 * esize)) == BADARG   # out on an operand
    assert named(desc((5, 8), (4, 8)), C.c_void_p(b.value + 31 * esize)) == "none" != named(desc((5, 8), (4, 8)), C.c_void_p(b.value + 32 * esize))
    for p in (0.0, 0.5, 3.0, -1.0):
        assert call(desc((5, 8), (4, 8), p=p)) == UNSUPPORTED, p
    bad = desc((5, 8), (4, 8))
    bad.mode = 3
    assert call(bad) == UNSUPPORTED
    assert call(desc((1 << 16, 8), (1 << 15, 8))) == UNSUPPORTED                                           # 2^31 outputs
    assert call(desc((1 << 20, 8), (4, 8), x1_ld=(1 << 11) + 1)) == UNSUPPORTED and call(desc((2, 1 << 27, 8), (4, 8))) == UNSUPPORTED
    assert hipops.cdist_kernel_name((5, 8), (4, 8), p=3.0) == "none" and hipops.cdist_kernel_name((1 << 16, 8), (1 << 15, 8)) == "none"


def test_kernel_name_at_the_mode_and_vector_boundaries(native_libs):
    H, _ = native_libs
    name, K, f32, f16 = hipops.cdist_kernel_name, cr.kname, np.float32, np.float16
    # torch's rule: P > 25 || R > 25
    assert name((25, 8), (25, 8)) == K("direct", f32, 2.0)
    assert name((26, 8), (1, 8)) == name((1, 8), (26, 8)) == name((3, 1, 8), (26, 8)) == K("mm", f32, True)
    assert name((2, 8), (2, 8), compute_mode="use_mm_for_euclid_dist") == K("mm", f32, True)
    assert name((64, 8), (64, 8), compute_mode="donot_use_mm_for_euclid_dist", half=True) == K("direct", f16, 2.0)
    for p in (1.0, INF):
        assert name((64, 8), (64, 8), p=p, compute_mode="use_mm_for_euclid_dist") == K("direct", f32, p)     # the mode is for p = 2 alone
    # the vector instantiation: m and the strides multiples of 4 (8 halves), the operands 16-byte aligned
    assert name((64, 4), (64, 4)) == K("mm", f32, True) and name((64, 6), (64, 6)) == K("mm", f32, False)
    assert name((64, 8), (64, 8), half=True) == K("mm", f16, True) and name((64, 12), (64, 12), half=True) == K("mm", f16, False)
    assert name((64, 8), (64, 8), x1_ld=9) == name((64, 8), (64, 8), x2_ld=10) == K("mm", f32, False)
    assert name((64, 8), (64, 8), x1_ld=12, out_ld=65) == K("mm", f32, True) and name((64, 8), (64, 8), x2_ld=12, half=True) == K("mm", f16, False)
    d = hipops.cdist_desc((64, 8), (64, 8))
    q = lambda a, b, half=0: H.si_hip_cdist_kernel_name(C.byref(d), C.c_void_p(a), C.c_void_p(b), C.c_void_p(1 << 42), half).decode()
    base = 1 << 40
    assert q(base, 2 * base) == K("mm", f32, True) and q(base + 4, 2 * base) == q(base, 2 * base + 8) == K("mm", f32, False)
    assert q(base + 8, 2 * base, 1) == K("mm", f16, False)


def test_plan_and_batch_rule_stand_alone_under_sanitizers(tmp_path):
    exe = str(tmp_path / "test_cdist_plan")
    subprocess.check_call(["g++", "-std=c++17", "-O0", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-static-libasan", "-static-libubsan", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "simpleinfer_amd", "csrc", "hip"),
                           "-I" + os.path.join(ROOT, "simpleinfer_amd", "csrc", "host"), os.path.join(ROOT, "tests", "cpp", "test_cdist_plan.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "cdist plan ok" in r.stdout and "runtime error" not in r.stderr, r.stdout[-4000:] + r.stderr[-4000:]
