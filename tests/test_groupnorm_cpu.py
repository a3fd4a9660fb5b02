"""CPU: nn.GroupNorm / nn.InstanceNorm2d -- the float64 numpy reference pinned to torch, the generator's lines, the toy U-Net's
default output pinned to what it was before the norm= / act= keywords existed, and the C-ABI of include/si_norm.h: exported,
bound under its own table, absent from include/si_hip.h, and every compute entry of it driven by the GPU file's view cases."""
import ctypes as C
import hashlib
import os
import re

import numpy as np
import pytest

import containment as ct
import gn_reference as gr
from ct_reference import _parse
from simpleinfer_amd import engine, hipops, modelgen as mg

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
NORM_HEADER = os.path.join(ROOT, "include", "si_norm.h")


@pytest.mark.parametrize("affine", [True, False], ids=["affine", "plain"])
@pytest.mark.parametrize("s", gr.SHAPES + gr.EXTRA_SHAPES + [gr.HALF_SHAPES[-1]], ids=gr.shape_id)
def test_numpy_reference_equals_torch(s, affine):
    torch = pytest.importorskip("torch")
    F = torch.nn.functional
    x, gamma, beta = gr.operands(s, 1, offset=0.25)
    n, h, w, c, g = s
    t = torch.from_numpy(x.astype(np.float64)).permute(0, 3, 1, 2)
    wt = torch.from_numpy(gamma.astype(np.float64)) if affine else None
    bt = torch.from_numpy(beta.astype(np.float64)) if affine else None
    ref = gr.group_norm_ref(x, g, gamma if affine else None, beta if affine else None, 1e-5)
    if h * w * (c // g) == 1:   # torch refuses one value per group; the definition gives beta exactly
        assert np.array_equal(ref, np.broadcast_to(np.float64(beta) if affine else 0.0, ref.shape))
        return
    got = F.group_norm(t, g, wt, bt, 1e-5).permute(0, 2, 3, 1).numpy()
    assert got.shape == ref.shape and np.abs(got - ref).max() <= 1e-12 * max(np.abs(ref).max(), 1.0)
    if g == c and h * w > 1:   # (torch refuses instance_norm on one value per channel)
        inst = F.instance_norm(t, None, None, wt, bt, True, 0.0, 1e-5).permute(0, 2, 3, 1).numpy()
        assert np.abs(inst - ref).max() <= 1e-12 * max(np.abs(ref).max(), 1.0)


def test_reference_activations():
    y = np.linspace(-4, 4, 33)
    assert np.array_equal(gr.act_ref(y, "relu"), np.maximum(y, 0))
    assert np.allclose(gr.act_ref(y, "silu"), y / (1 + np.exp(-y)), rtol=0, atol=1e-15)
    assert np.array_equal(gr.act_ref(y, "leakyrelu", 0.1), np.where(y > 0, y, 0.1 * y))
    x, gamma, beta = gr.operands((1, 3, 3, 4, 2))
    assert np.array_equal(gr.group_norm_ref(x, 2, gamma, beta, act="relu"), np.maximum(gr.group_norm_ref(x, 2, gamma, beta), 0))


def test_builders_emit_pnnx_keys():
    b = mg.PnnxBuilder(seed=1)
    x = b.input((2, 12, 5, 7))
    y = b.group_norm(x, 4, eps=1e-3)
    z = b.instance_norm(y)
    zz = b.instance_norm(z, affine=True, track_running_stats=True)
    b.output(zz)
    lines = {p[0] + ":" + p[1]: p for p in (_parse(ln) for ln in b.lines)}
    typ, name, ins, outs, prm = lines["nn.GroupNorm:gn_0"]
    assert prm == dict(affine="True", eps="%e" % 1e-3, num_channels="12", num_groups="4") and (ins, outs) == ([x], [y])
    assert b.attrs["gn_0.weight"].shape == (12,) and b.attrs["gn_0.bias"].shape == (12,)
    assert "@weight=(12)f32" in b.lines[1] and "@bias=(12)f32" in b.lines[1]
    typ, name, ins, outs, prm = lines["nn.InstanceNorm2d:in_0"]
    assert prm == dict(affine="False", eps="%e" % 1e-5, num_features="12", track_running_stats="False")
    assert "in_0.weight" not in b.attrs and "@" not in b.lines[2]
    typ, name, ins, outs, prm = lines["nn.InstanceNorm2d:in_1"]
    assert prm == dict(affine="True", eps="%e" % 1e-5, num_features="12", track_running_stats="True")
    assert b.attrs["in_1.weight"].shape == (12,) and b.attrs["in_1.bias"].shape == (12,)
    assert b.shapes[zz] == (2, 12, 5, 7)
    with pytest.raises(AssertionError):
        b.group_norm(x, 5)


def _digest(b):
    h = hashlib.sha256()
    for ln in b.lines:
        h.update(ln.encode() + b"\n")
    for k in sorted(b.attrs):
        h.update(k.encode())
        h.update(b.attrs[k].tobytes())
    return h.hexdigest()


# sha256 over the lines and the attributes (sorted by name) of build_toy_unet() / build_toy_unet(up="bilinear") as the parent commit wrote them
PARENT_UNET = {"convtranspose": "37f3669d91412b115ab8908fc932dfc56178f5a4daeb9f00832f12ffa827db4b",
               "bilinear": "b6d9d3c79c06bb58ee0c81fa283829972e0096d9692ec236f1d77be4472f0247"}


@pytest.mark.parametrize("up", sorted(PARENT_UNET))
def test_toy_unet_defaults_are_unchanged(up):
    a, b = mg.build_toy_unet(up=up), mg.build_toy_unet(up=up, norm="bn", act="relu")
    assert a.lines == b.lines and sorted(a.attrs) == sorted(b.attrs)
    assert all(np.array_equal(a.attrs[k], b.attrs[k]) for k in a.attrs)
    assert _digest(a) == PARENT_UNET[up]


def test_toy_unet_variants():
    gn = mg.build_toy_unet(norm="gn", act="silu")
    types = [ln.split()[0] for ln in gn.lines]
    assert types.count("nn.GroupNorm") == 14 and types.count("nn.SiLU") == 14 and "nn.BatchNorm2d" not in types and "nn.ReLU" not in types
    inn = mg.build_toy_unet(norm="in")
    types = [ln.split()[0] for ln in inn.lines]
    assert types.count("nn.InstanceNorm2d") == 14 and types.count("nn.ReLU") == 14 and "nn.BatchNorm2d" not in types
    assert not any(k.startswith("in_") for k in inn.attrs)   # no affine
    # the float64 evaluation handles both
    x = mg.synth_input((1, 16, 16, 3))
    for b in (mg.build_toy_unet(batch=1, size=16, norm="gn", act="silu"), mg.build_toy_unet(batch=1, size=16, norm="in")):
        y = gr.eval_graph(b, x)
        assert y.shape == (1, 16, 16, 4) and np.isfinite(y).all()
    with pytest.raises(AssertionError):
        mg.build_toy_unet(norm="ln")


def _declared(path):
    src = open(path).read()
    src = re.sub(r"/\*.*?\*/", " ", src, flags=re.S)
    src = re.sub(r"//[^\n]*", " ", src)
    names = []
    for m in re.finditer(r"\b(si_[a-z0-9_]+)\s*\(", src):
        if m.group(1) not in names:
            names.append(m.group(1))
    return names


def test_norm_header_is_exported_and_bound(native_libs):
    H, _ = native_libs
    declared = _declared(NORM_HEADER)
    assert declared == ["si_hip_groupnorm_workspace_bytes", "si_hip_groupnorm_f32", "si_hip_groupnorm_f16", "si_hip_groupnorm_kernel_name"]
    assert sorted(H._si_norm_signatures) == sorted(declared)
    assert not set(declared) & set(H._si_signatures)
    from simpleinfer_amd import _native
    raw = C.CDLL(_native.LIB_HIP_PATH)   # a handle of its own: nothing but the dynamic symbol table answers
    missing = [name for name in declared if not hasattr(raw, name)]
    assert not missing, missing
    for name in declared:
        assert getattr(H, name).argtypes is not None


def test_si_hip_header_declares_none_of_them():
    text = open(ct.HEADER).read()
    for name in _declared(NORM_HEADER):
        assert name not in text, name
    assert "groupnorm" not in text.lower()


def test_registry_lists_both_types(native_libs):
    types = engine.registry_types()
    assert "nn.GroupNorm" in types and "nn.InstanceNorm2d" in types
    assert "nn.GELU" not in types


def test_every_compute_entry_of_the_norm_header_is_driven():
    """the rule of tests/test_containment_cpu.py for include/si_hip.h, applied to include/si_norm.h and the view cases of the GPU file"""
    import test_gpu_groupnorm as tg
    entries = [n for n in ct.header_functions(NORM_HEADER) if not ct.is_exempt(n)]
    assert entries == ["si_hip_groupnorm_f32", "si_hip_groupnorm_f16"]
    driven = {e for c in tg.VIEW_CASES for e in c.entries}
    assert set(entries) <= driven, sorted(set(entries) - driven)
    assert driven <= set(ct.header_functions(NORM_HEADER)), "a case names an entry the header does not declare"


def test_abi_without_a_device(native_libs):
    """refusals happen before any device call (the pointers are never looked at), and the form / workspace follow the shape alone"""
    H, _ = native_libs
    dummy = C.c_void_p(256)

    def call(d, gamma=dummy, beta=dummy, ws=dummy, fn="si_hip_groupnorm_f32", src=dummy, dst=dummy):
        return getattr(H, fn)(C.byref(d), src, gamma, beta, dst, ws, None)

    shape = (2, 48, 40, 32)
    for fn in ("si_hip_groupnorm_f32", "si_hip_groupnorm_f16"):
        assert call(hipops.group_norm_desc(shape, 5), fn=fn) == -1                      # c % groups
        assert call(hipops.group_norm_desc(shape, 0), fn=fn) == -1
        assert call(hipops.group_norm_desc(shape, 4, in_ld=31), fn=fn) == -1            # ld < c
        assert call(hipops.group_norm_desc(shape, 4, out_ld=16), fn=fn) == -1
        assert call(hipops.group_norm_desc(shape, 4, affine=True), gamma=None, fn=fn) == -1
        assert call(hipops.group_norm_desc(shape, 4, affine=True), beta=None, fn=fn) == -1
        assert call(hipops.group_norm_desc(shape, 4), ws=None, fn=fn) == -1             # a null workspace where bytes > 0
        assert call(hipops.group_norm_desc(shape, 4), src=None, fn=fn) == -1
        assert call(hipops.group_norm_desc(shape, 4), dst=None, fn=fn) == -1
        bad = hipops.group_norm_desc(shape, 4)
        bad.act = 7
        assert call(bad, fn=fn) == -1
        assert call(hipops.group_norm_desc((65536, 256, 128, 8), 2), fn=fn) == -2       # n * h * w = 2^31
        assert getattr(H, fn)(None, dummy, dummy, dummy, dummy, dummy, None) == -1
    assert hipops.group_norm_workspace_bytes(shape, 4) == 2 * 8 * 4 * 8                  # [n][8 slices][4 groups] float pairs
    assert hipops.group_norm_workspace_bytes((1, 8, 8, 1024), 32) == 0
    assert hipops.group_norm_workspace_bytes(shape, 5) == 0
    assert hipops.group_norm_kernel_name(shape, 5) == "none"
    # the slice count comes from h * w alone
    assert hipops.group_norm_workspace_bytes((3, 48, 40, 64), 64) == 3 * 8 * 64 * 8
    assert hipops.group_norm_workspace_bytes((1, 256, 256, 8), 1) == 32 * 8
    # the form follows the shape, the vector width the strides and the pointers
    assert hipops.group_norm_kernel_name((1, 8, 8, 1024), 32) == "groupnorm_slab_kernel<float, 4>"
    assert hipops.group_norm_kernel_name((2, 12, 10, 12), 4, half=True) == "groupnorm_slab_kernel<_Float16, 1>"
    assert hipops.group_norm_kernel_name(shape, 4, half=True) == "groupnorm_stats_kernel<_Float16, 8> + groupnorm_apply_kernel<_Float16, 8>"
    assert hipops.group_norm_kernel_name(shape, 4, in_ld=33).endswith("<float, 1>")
    d = hipops.group_norm_desc(shape, 4)
    assert H.si_hip_groupnorm_kernel_name(C.byref(d), C.c_void_p(260), dummy, 0).decode().endswith("<float, 1>")
