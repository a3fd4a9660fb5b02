"""CPU: nn.ConvTranspose2d -- the fp64 numpy reference pinned to torch, the toy U-Net file pinned to the reference's own pnnx
loader, and the new C-ABI entry points that need no device."""
import ctypes as C
import os

import numpy as np
import pytest

import util
from ct_reference import SHAPES, conv_transpose2d_ref, eval_graph, operands, shape_id
from simpleinfer_amd import engine, hipops, modelgen as mg

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
REF_BIN = os.path.join(ROOT, "oracle", "_ref", "ref_pnnx_dump")


@pytest.mark.parametrize("s", SHAPES, ids=[shape_id(s) for s in SHAPES])
def test_numpy_reference_equals_torch(s):
    torch = pytest.importorskip("torch")
    k, st, p, op, d, _, _ = s
    x, wt, b = operands(s)
    ref = conv_transpose2d_ref(x, wt, b, st, p, op, d)
    t = torch.nn.functional.conv_transpose2d(torch.from_numpy(x.astype(np.float64)).permute(0, 3, 1, 2), torch.from_numpy(wt.astype(np.float64)),
                                             torch.from_numpy(b.astype(np.float64)), stride=st, padding=p, output_padding=op, dilation=d)
    got = t.permute(0, 2, 3, 1).numpy()
    assert got.shape == ref.shape
    assert np.abs(got - ref).max() <= 1e-12 * np.abs(ref).max()


def test_toy_unet_loads_like_the_reference_loader(native_libs, tmp_path):
    """the .param / .bin pair of build_toy_unet through the product loader equals the reference's own loader's dump"""
    if not os.path.exists(REF_BIN):
        pytest.skip("oracle/_ref/ref_pnnx_dump is not built here")
    import subprocess
    pp, bp = str(tmp_path / "u.pnnx.param"), str(tmp_path / "u.pnnx.bin")
    mg.build_toy_unet().save(pp, bp)
    for expand in (False, True):
        out = str(tmp_path / "dump.txt")
        engine.pnnx_dump(pp, bp, expand, out)
        ours = open(out).read()
        ref = subprocess.run([REF_BIN, pp, bp] + (["--expand"] if expand else []), check=True, capture_output=True, text=True).stdout
        assert "nn.ConvTranspose2d" in ours
        assert ours == ref


def test_toy_unet_fp32_evaluation_is_within_the_bar():
    """The condition of the GPU U-Net test: a torch float32 CPU evaluation of the chosen graph and input is itself within REL_TOL of the fp64
    evaluation (both metrics), so an fp32 engine can be held to that bar on this graph."""
    torch = pytest.importorskip("torch")
    F = torch.nn.functional
    b = mg.build_toy_unet()
    x = mg.synth_input((2, 64, 64, 3))
    ref = eval_graph(b, x)
    vals = {}
    from ct_reference import _parse, _ints
    for typ, name, ins, outs, prm in (_parse(ln) for ln in b.lines):
        a = lambda k: torch.from_numpy(b.attrs["%s.%s" % (name, k)])
        if typ == "pnnx.Input":
            vals[outs[0]] = torch.from_numpy(x).permute(0, 3, 1, 2).contiguous()
            continue
        if typ == "pnnx.Output":
            got = vals[ins[0]].permute(0, 2, 3, 1).numpy()
            continue
        t = vals[ins[0]]
        if typ == "nn.Conv2d":
            y = F.conv2d(t, a("weight"), a("bias"), stride=_ints(prm["stride"]), padding=_ints(prm["padding"]))
        elif typ == "nn.ConvTranspose2d":
            y = F.conv_transpose2d(t, a("weight"), a("bias"), stride=_ints(prm["stride"]), padding=_ints(prm["padding"]),
                                   output_padding=_ints(prm["output_padding"]), dilation=_ints(prm["dilation"]))
        elif typ == "nn.BatchNorm2d":
            y = F.batch_norm(t, a("running_mean"), a("running_var"), a("weight"), a("bias"), False, 0.0, float(prm["eps"]))
        elif typ == "nn.ReLU":
            y = F.relu(t)
        elif typ == "nn.MaxPool2d":
            y = F.max_pool2d(t, 2, 2)
        elif typ == "torch.cat":
            y = torch.cat([vals[i] for i in ins], 1)
        vals[outs[0]] = y
    assert got.dtype == np.float32
    e = util.rel_err(got, ref)
    m = util.mixed_err(got, ref)
    print("torch float32 vs fp64 on the toy U-Net: max-based %.3e, element-wise %.3e" % (e, m))
    assert e <= util.REL_TOL and m <= util.REL_TOL


def test_abi_without_a_device(native_libs):
    H, _ = native_libs
    for name in ("si_hip_conv_transpose2d_weight_elems", "si_hip_conv_transpose2d_pack_weight_host", "si_hip_conv_transpose2d_f32",
                 "si_hip_conv_transpose2d_kernel_name"):
        assert hasattr(H, name), name
    x_shape, w_shape = (2, 10, 14, 30), (30, 48, 3, 3)
    d = hipops.conv_transpose2d_desc(x_shape, w_shape, True, (2, 2), (1, 1), (1, 1))
    assert (d.oh, d.ow) == (20, 28)
    # a wrong oh is refused before any device call (pointers are never looked at)
    bad = hipops.conv_transpose2d_desc(x_shape, w_shape, True, (2, 2), (1, 1), (1, 1))
    bad.oh += 1
    dummy = C.c_void_p(16)
    assert H.si_hip_conv_transpose2d_f32(C.byref(bad), dummy, dummy, dummy, dummy, None) == -1   # SI_E_BADARG
    grp = hipops.conv_transpose2d_desc(x_shape, w_shape, True, (2, 2), (1, 1), (1, 1))
    grp.groups = 2
    assert H.si_hip_conv_transpose2d_f32(C.byref(grp), dummy, dummy, dummy, dummy, None) == -2   # SI_E_UNSUPPORTED
    # the weight image: exactly weight_elems elements, a permutation of the input plus zero padding
    rng = np.random.default_rng(3)
    w = rng.uniform(0.5, 1.5, w_shape).astype(np.float32) * rng.choice([-1.0, 1.0], w_shape).astype(np.float32)
    elems = H.si_hip_conv_transpose2d_weight_elems(C.byref(d))
    assert elems == 3 * 3 * 48 * 32
    buf = np.full(elems + 64, np.float32(7.25), np.float32)
    assert H.si_hip_conv_transpose2d_pack_weight_host(C.byref(d), w.ctypes.data_as(C.c_void_p), buf.ctypes.data_as(C.c_void_p)) == 0
    assert (buf[elems:] == np.float32(7.25)).all(), "wrote past weight_elems"
    packed = buf[:elems]
    nz = packed[packed != 0]
    assert nz.size == w.size and np.array_equal(np.sort(nz), np.sort(w.ravel()))
    assert (packed == 0).sum() == elems - w.size
