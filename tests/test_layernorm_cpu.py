"""CPU: F.layer_norm / F.gelu -- the float64 rules pinned to torch float64, the builder's lines and the toy, the registry, the refusals and form
boundaries of include/si_layernorm.h without a device, and the batch rule as a stand-alone C++ program under ASan and UBSan (a child process)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import layernorm_reference as lnr
from ct_reference import _parse
from simpleinfer_amd import engine, hipops, modelgen as mg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BADARG, UNSUPPORTED = -1, -2
F = torch.nn.functional


@pytest.mark.parametrize("approximate", ["none", "tanh"])
@pytest.mark.parametrize("affine", ["both", "none", "weight"])
@pytest.mark.parametrize("shape", [(5, 24), (3, 7, 33)], ids=["rank2", "rank3"])
def test_rules_are_torch_float64(shape, affine, approximate):
    r = np.random.RandomState(3)
    x = 3.0 + 0.5 * r.standard_normal(shape)
    g = r.uniform(0.5, 1.5, shape[-1]) if affine != "none" else None
    b = r.uniform(-0.5, 0.5, shape[-1]) if affine == "both" else None
    t = lambda a: None if a is None else torch.from_numpy(a)
    want = F.layer_norm(t(x), (shape[-1],), t(g), t(b), float(np.float32(1e-5))).numpy()
    assert np.abs(lnr.layernorm_ref(x, g, b, 1e-5) - want).max() <= 1e-12
    # (absolute: torch's 1 + erf form is 0 below x = -8.3 in float64, where the rule's erfc form still has the tail)
    x = np.concatenate([np.linspace(-12, 12, 4801), [0.0, -0.0, 1e-30, -1e-30]])
    assert np.abs(lnr.gelu_ref(x, approximate) - F.gelu(t(x), approximate=approximate).numpy()).max() <= 1e-12


def test_builder_lines_and_the_toy():
    b = mg.PnnxBuilder(seed=1)
    x = b.input((2, 16, 32))
    z = b.layer_norm(b.layer_norm(x), weight=True, bias=False, eps=1e-6)
    b.output(b.gelu(b.gelu(b.layer_norm(z, weight=False, bias=False)), "tanh"))
    ops = [_parse(ln) for ln in b.lines]
    assert [o[0] for o in ops] == ["pnnx.Input", "pnnx.Attribute", "pnnx.Attribute", "F.layer_norm", "pnnx.Attribute", "F.layer_norm", "F.layer_norm",
                                   "F.gelu", "F.gelu", "pnnx.Output"]
    full, weight_only, bare = ops[3], ops[5], ops[6]
    assert len(full[2]) == 3 and full[4]["normalized_shape"] == "(32)" and float(full[4]["eps"]) == 1e-5 and "weight" not in full[4]
    assert len(weight_only[2]) == 2 and weight_only[4]["bias"] == "None" and "weight" not in weight_only[4] and float(weight_only[4]["eps"]) == 1e-6
    assert len(bare[2]) == 1 and bare[4]["weight"] == bare[4]["bias"] == "None"
    assert ops[7][4] == {"approximate": "none"} and ops[8][4] == {"approximate": "tanh"}
    assert b.attrs[ops[1][1] + ".data"].shape == b.attrs[ops[2][1] + ".data"].shape == (32,)
    # the toy: conv -> permute -> view, per layer LN MHA add LN Linear GELU Linear add, then LN Linear
    toy = mg.build_toy_vit_block(2, 16, 32, 4, 2)
    seq = [_parse(ln)[0] for ln in toy.lines if not ln.startswith("pnnx.Attribute")]
    layer = ["F.layer_norm", "nn.MultiheadAttention", "pnnx.Expression", "F.layer_norm", "nn.Linear", "F.gelu", "nn.Linear", "pnnx.Expression"]
    assert seq == ["pnnx.Input", "nn.Conv2d", "Tensor.permute", "Tensor.view"] + layer * 2 + ["F.layer_norm", "nn.Linear", "pnnx.Output"]
    assert toy.shapes[_parse(toy.lines[-1])[2][0]] == (2, 16, 10)
    mha = [_parse(ln) for ln in toy.lines if ln.startswith("nn.MultiheadAttention")][0]
    assert mha[4]["batch_first"] == "True" and mha[4]["num_heads"] == "4" and toy.shapes[mha[2][0]] == (2, 16, 32)


def test_registry_and_abi_refusals_without_a_device(native_libs):
    """refusals happen before any device call (the pointers are compared, never followed); the registry holds the functional spellings only"""
    H, _ = native_libs
    types = engine.registry_types()
    assert "F.layer_norm" in types and "F.gelu" in types and "nn.LayerNorm" not in types and "nn.GELU" not in types
    src, dst = C.c_void_p(1 << 20), C.c_void_p(1 << 40)
    desc = hipops.layernorm_desc
    for fn in ("si_hip_layernorm_f32", "si_hip_layernorm_f16"):
        esize = 4 if fn.endswith("f32") else 2
        call = lambda d, a=src, b=dst: getattr(H, fn)(C.byref(d), a, None, None, b, None)
        assert getattr(H, fn)(None, src, None, None, dst, None) == BADARG
        assert call(desc(6, 8), a=None) == BADARG and call(desc(6, 8), b=None) == BADARG
        for field in ("rows", "c", "in_ld", "out_ld"):
            for value in (0, -3):
                bad = desc(6, 8)
                setattr(bad, field, value)
                assert call(bad) == BADARG, (field, value)
        assert call(desc(6, 8, in_ld=7)) == BADARG and call(desc(6, 8, out_ld=7)) == BADARG
        assert call(desc(6, 8, eps=-1e-5)) == BADARG and call(desc(6, 8, eps=float("nan"))) == BADARG
        assert call(desc(6, 8), a=src, b=src) == BADARG                                                    # overlapping views
        assert call(desc(6, 8), a=src, b=C.c_void_p(src.value + 5 * esize)) == BADARG
        assert call(desc(6, 8, in_ld=16, out_ld=16), a=src, b=C.c_void_p(src.value + 4 * esize)) == BADARG   # channels 4 .. 11 meet 0 .. 7
        assert call(desc(1 << 20, 8, out_ld=1 << 11)) == UNSUPPORTED                                       # offsets of 2^31, one side
        assert call(desc(1 << 28, 8)) == UNSUPPORTED
    name = hipops.layernorm_kernel_name
    assert name(6, 8, in_ld=7) == "none" and name(0, 8) == "none" and name(1 << 28, 8) == "none"
    assert name(6, 8, in_ld=16, out_ld=16) == lnr.kname("row_group", np.float32, True)                     # disjoint slices are served


def test_kernel_name_at_the_form_boundaries(native_libs):
    H, _ = native_libs
    name, K = hipops.layernorm_kernel_name, lnr.kname
    f32, f16 = np.float32, np.float16
    for c, form in ((8, "row_group"), (1024, "row_group"), (1028, "row_block"), (4096, "row_block"), (4100, "row_block_3pass")):
        assert name(3, c) == K(form, f32, True) == lnr.expected_kernel(c, f32, True), c
        assert name(3, c, half=True) == K(form, f16, c % 8 == 0), c
        assert name(3, c + 1) == lnr.expected_kernel(c + 1, f32, False) and name(3, c + 1).endswith("<float, 1>"), c
    # c, either stride and either pointer decide the instantiation
    assert name(3, 8, in_ld=9) == K("row_group", f32, False) and name(3, 8, out_ld=12, half=True) == K("row_group", f16, False)
    d = hipops.layernorm_desc(3, 8)
    q = lambda a, b, half: H.si_hip_layernorm_kernel_name(C.byref(d), C.c_void_p(a), C.c_void_p(b), half).decode()
    assert q(256, 512, 0) == K("row_group", f32, True) and q(260, 512, 0) == K("row_group", f32, False) and q(256, 520, 1) == K("row_group", f16, False)


def test_batch_rule_for_layer_norm_and_gelu_stand_alone_under_sanitizers(tmp_path):
    exe = str(tmp_path / "test_batch_rule_layernorm")
    subprocess.check_call(["g++", "-std=c++17", "-O0", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-static-libasan", "-static-libubsan", "-I" + os.path.join(ROOT, "simpleinfer_amd", "csrc", "host"),
                           os.path.join(ROOT, "tests", "cpp", "test_batch_rule_layernorm.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "layernorm rule ok" in r.stdout and "runtime error" not in r.stderr, r.stdout[-4000:] + r.stderr[-4000:]
