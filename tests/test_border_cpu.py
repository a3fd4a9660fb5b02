"""CPU: the border-mapped convolution's host side (include/si_border.h) -- the coordinate map against numpy's pad, the float64 restatement of
tests/border_reference.py against torch's own nn.Conv2d(padding_mode=...), every refusal of the C-ABI by return code without a launch, and
the builder's nn.Conv2d line."""
import ctypes as C

import numpy as np
import pytest

import border_reference as br
from ct_reference import _parse
from simpleinfer_amd import hipops, modelgen as mg

BADARG, UNSUPPORTED = -1, -2


@pytest.mark.parametrize("mode", sorted(br.NP_MODE))
def test_source_index_is_numpys_pad(native_libs, mode):
    H, _ = native_libs
    refused, code = br.ENUMS["SI_BORDER_REFUSED"], hipops.PAD_MODE[mode]
    for n in range(1, 10):
        limit = {"replicate": n + 3, "reflect": n - 1, "circular": n}[mode]
        for pad in range(limit + 1):
            want = np.pad(np.arange(n), pad, br.NP_MODE[mode])
            got = [H.si_hip_conv2d_border_source_index(code, i, n) for i in range(-pad, n + pad)]
            assert got == list(want), (mode, n, pad)
        if mode != "replicate":     # one step beyond the precondition on either side
            assert H.si_hip_conv2d_border_source_index(code, -limit - 1, n) == refused
            assert H.si_hip_conv2d_border_source_index(code, n + limit, n) == refused
    assert H.si_hip_conv2d_border_source_index(code, 0, 0) == refused and H.si_hip_conv2d_border_source_index(hipops.PAD_MODE["constant"], 0, 4) == refused


@pytest.mark.parametrize("case", br.CASES, ids=br.case_id)
def test_reference_equals_torch_conv2d_module(case):
    torch = pytest.importorskip("torch")
    n, c, h, wd, oc, k, s, p, d, mode = case
    x, w, b = br.operands(case, seed=3)
    m = torch.nn.Conv2d(c, oc, br.pair(k), br.pair(s), br.pair(p), br.pair(d), padding_mode=mode, dtype=torch.float64)
    with torch.no_grad():
        m.weight.copy_(torch.from_numpy(w.astype(np.float64)))
        m.bias.copy_(torch.from_numpy(b.astype(np.float64)))
        want = m(torch.from_numpy(x.astype(np.float64))).numpy()
    got = br.conv2d_border_ref(x, w, b, s, p, d, mode)
    assert got.shape == want.shape and np.abs(got - want).max() <= 1e-12


# (code, descriptor arguments, fields overwritten afterwards): every refusal of the header, one row each
X4 = (1, 4, 6, 8)
REFUSALS = [(BADARG, {}, {f: v}) for f in ("n", "ih", "iw", "ic", "oh", "ow", "oc", "kh", "kw", "sh", "sw", "dh", "dw", "groups") for v in (0, -1)] + [
    (BADARG, {}, {f: v}) for f, v in (("pt", -1), ("pl", -1), ("in_ld", 7), ("out_ld", 23), ("mode", 0), ("mode", 4), ("oh", 8), ("ow", 12))] + [
    (UNSUPPORTED, dict(xs=X4, k=9, padding=(4, 4), mode="reflect"), {}),                    # reflect pad = H
    (UNSUPPORTED, dict(xs=(1, 6, 4, 8), k=9, padding=(4, 4), mode="reflect"), {}),          # reflect pad = W
    (UNSUPPORTED, dict(xs=(1, 3, 6, 8), k=9, padding=(4, 4), mode="circular"), {}),         # circular pad = H + 1
    (UNSUPPORTED, dict(groups=2), {}),
    (UNSUPPORTED, dict(xs=(3, 9, 11, 8), in_ld=1 << 25), {}), (UNSUPPORTED, dict(xs=(3, 9, 11, 8), out_ld=1 << 25), {}),   # offsets beyond 31 bits
    (UNSUPPORTED, dict(xs=(65536, 1, 1, 8), oc=1), {}),                                     # batch beyond a grid's z
    (UNSUPPORTED, dict(xs=(1, 200, 200, 8), dilation=(90, 90), padding=(90, 90)), {}),      # a patch beyond LDS
]
ACCEPTED = [dict(), dict(residual=True, in_ld=16, out_ld=40, res_ld=32), dict(xs=X4, k=9, padding=(4, 4), mode="circular"),
            dict(xs=(1, 5, 5, 8), k=9, padding=(4, 4)), dict(xs=(1, 1, 1, 8), k=9, padding=(4, 4), mode="replicate"),
            dict(xs=(1, 64, 64, 8), k=5, stride=(2, 2), dilation=(2, 2), padding=(4, 4))]    # the last fits LDS with fewer live rows


@pytest.mark.parametrize("half", [0, 1], ids=["f32", "f16"])
def test_abi_refusals_without_a_launch(native_libs, half):
    """every refusal happens before any device call: the addresses are made up, 16-byte aligned and 16 MiB apart"""
    H, _ = native_libs
    X, W, B, R, Y = (C.c_void_p((j + 1) << 24) for j in range(5))
    fn = H.si_hip_conv2d_border_f16 if half else H.si_hip_conv2d_border_f32

    def desc(xs=(2, 9, 11, 8), oc=24, k=3, **kw):
        return hipops.conv2d_border_desc(xs, (oc, xs[3], k, k), **kw)

    def call(dd, x=X, w=W, b=B, r=R, y=Y):
        return fn(C.byref(dd), x, w, b, r, y, None)

    def name(dd, x=X, y=Y):
        return H.si_hip_conv2d_border_kernel_name(C.byref(dd), x, y, half)

    for code, args, fields in REFUSALS:
        dd = desc(**args)
        for f, v in fields.items():
            setattr(dd, f, v)
        assert call(dd) == code and name(dd) == b"none" and H.si_hip_conv2d_border_supported(C.byref(dd), half) == 0, (code, args, fields)
    for args in ACCEPTED:
        assert name(desc(**args)) == (b"conv_border_kernel<_Float16>" if half else b"conv_border_kernel<float>"), args
        assert H.si_hip_conv2d_border_supported(C.byref(desc(**args)), half) == 1
    # pointers: null, y over an input, off their element
    assert fn(None, X, W, B, R, Y, None) == BADARG and H.si_hip_conv2d_border_kernel_name(None, X, Y, half) == b"none"
    es = 2 if half else 4
    for kw in (dict(x=None), dict(w=None), dict(y=None), dict(b=None), dict(y=X), dict(y=W), dict(y=B), dict(y=C.c_void_p(X.value + 2 * 9 * 11 * 8 * es - es))):
        assert call(desc(), **kw) == BADARG, kw
    assert call(desc(residual=True), r=None) == BADARG and call(desc(bias=False), b=None) != BADARG
    assert call(desc(), x=C.c_void_p(X.value + 1)) == UNSUPPORTED and name(desc(), x=C.c_void_p(X.value + 1)) == b"none"
    assert call(desc(), w=C.c_void_p(W.value + 8)) == UNSUPPORTED
    # the channel rule of fp16 alone, and no weight image for it
    d12 = desc((2, 9, 11, 12))
    assert H.si_hip_conv2d_border_supported(C.byref(d12), half) == 1 - half and (call(d12) == UNSUPPORTED) == bool(half)
    assert H.si_hip_conv2d_border_weight_elems(C.byref(d12), half) == (0 if half else 24 * 9 * 12)


def test_builder_line_carries_the_mode_and_the_default_is_unchanged():
    def line(**kw):
        b = mg.PnnxBuilder(seed=1)
        b.conv(b.input((1, 4, 8, 8)), 6, 3, 1, 1, **kw)
        return b.lines[-1]

    default = line()
    assert _parse(default)[4]["padding_mode"] == "zeros" and line(padding_mode="zeros") == default
    assert default == ("nn.Conv2d conv_0 1 1 0 1 bias=True dilation=(1,1) groups=1 in_channels=4 kernel_size=(3,3) out_channels=6 padding=(1,1) "
                       "padding_mode=zeros stride=(1,1) @weight=(6,4,3,3)f32 @bias=(6)f32 #0=(1,4,8,8)f32 #1=(1,6,8,8)f32")
    for mode in ("reflect", "replicate", "circular"):
        assert line(padding_mode=mode) == default.replace("padding_mode=zeros", "padding_mode=" + mode)
    # the generator's two spellings: the same convolutions by name and weights, no pad layers in the second
    a, b = mg.build_toy_cyclegan(), mg.build_toy_cyclegan(in_conv=True)
    convs = lambda g: [_parse(ln) for ln in g.lines if ln.startswith("nn.Conv2d")]
    assert [c[1] for c in convs(a)] == [c[1] for c in convs(b)] and not [ln for ln in b.lines if "Pad2d" in ln or ln.startswith("F.pad")]
    assert [c[4]["padding_mode"] for c in convs(b)] == ["reflect", "zeros", "zeros"] + ["reflect"] * 5
    assert all(np.array_equal(a.attrs[k], b.attrs[k]) for k in a.attrs) and sorted(a.attrs) == sorted(b.attrs)
