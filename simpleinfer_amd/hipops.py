"""numpy-in / numpy-out wrappers over the kernel C-ABI (include/si_hip.h).

Each helper uploads its operands to HBM, launches exactly one C-ABI kernel entry point and downloads
the result, so the parity tests exercise the same symbols a C / cgo / JNI caller would bind.  No
computation happens in Python; without a HIP device every call raises HipError.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence

import numpy as np

import contextlib

from . import _native
from ._native import SiConvPlan, SiPool2dDesc

# The kernel-form plan attached to every conv descriptor THIS MODULE builds (tests and sweeps hold every tile / form of a kernel family to the
# same bits through it).  State of this Python test helper only: the C-ABI itself has no process-global switch -- a plan travels inside the
# descriptor of one call (include/si_hip.h SiConv2dDesc::plan).
_PLAN = None


@contextlib.contextmanager
def plan(**fields):
    """with hipops.plan(f32_tile=4): ...  -- every conv launched through this module inside the block carries SiConvPlan(**fields)"""
    global _PLAN
    prev, _PLAN = _PLAN, SiConvPlan(**fields)
    try:
        yield _PLAN
    finally:
        _PLAN = prev


def set_plan(**fields):
    """the non-scoped form of plan(): every later conv launched through this module carries SiConvPlan(**fields); no fields = no plan"""
    global _PLAN
    _PLAN = SiConvPlan(**fields) if fields else None


def SiConv2dDesc(*a):
    d = _native.SiConv2dDesc(*a)
    if _PLAN is not None:
        d.plan = C.pointer(_PLAN)
    return d

# entry -> the kernel instantiation its *_kernel_name query named for the LAST launch through this module, asked with the pointers of that launch
# (the launchers choose kernels by pointer alignment: a guarded call must take the kernel of the plain one, tests/test_gpu_containment.py)
LAST_KERNEL_NAME = {}

ACT = {"none": 0, "relu": 1, "silu": 2, "sigmoid": 3, "hardsigmoid": 4, "hardswish": 5, "leakyrelu": 6}


class HipError(RuntimeError):
    pass


LAST_ENTRIES = []   # every si_hip_* function called through _chk since the list was last cleared, runtime calls included: the containment test
                    # keeps the compute entries of it (tests/containment.py is_exempt) and requires each label to be a function of the header


def _chk(rc: int, what: str):
    if what.startswith("si_hip_"):
        LAST_ENTRIES.append(what)
    if rc != 0:
        raise HipError("%s: %s (code %d)" % (what, _native.hip().si_hip_error_string(rc).decode(), rc))


class ContainmentError(RuntimeError):
    """a kernel touched memory outside the buffer it was given (guard_bands), or wrote to one of its inputs"""


class ByteFill:
    """a fill given as a byte pattern instead of a value: ByteFill(0xFF) is a NaN as fp32 and as fp16, 255 as u8; ByteFill(0x7B) is 1.3e36 as
    fp32, 61280 as fp16, 123 as u8 -- the two patterns of the containment tests (tests/containment.py)"""

    def __init__(self, byte: int):
        assert 0 <= int(byte) <= 255, byte
        self.byte = int(byte)

    def __repr__(self):
        return "ByteFill(0x%02X)" % self.byte


def _full(shape, dtype, fill) -> np.ndarray:
    """np.full for a value or a ByteFill"""
    if isinstance(fill, ByteFill):
        dt = np.dtype(dtype)
        return np.full(int(np.prod(shape, dtype=np.int64)) * dt.itemsize, fill.byte, np.uint8).view(dt).reshape(shape)
    return np.full(shape, fill, dtype)


_GUARD = None   # the active guard_bands() context, or None: state of this Python test helper only


def _creation_site() -> str:
    """function:line of the first frame outside DeviceBuffer / the view helpers: names a guarded buffer in a ContainmentError"""
    import sys
    f = sys._getframe(1)
    while f is not None and (f.f_code.co_name in ("__init__", "from_numpy", "_creation_site", "_view_in", "_view_out", "_range_flag", "<listcomp>")
                             and f.f_code.co_filename == __file__):
        f = f.f_back
    return "%s:%d" % (f.f_code.co_name, f.f_lineno) if f is not None else "?"


class GuardBands:
    """What guard_bands() yields: every DeviceBuffer created while it is active, with the bytes that must not change around (and, for inputs,
    inside) each of them.  check() compares; the first difference raises ContainmentError."""

    def __init__(self, pattern: int, nbytes: int):
        assert 0 <= pattern <= 255 and nbytes > 0 and nbytes % 256 == 0, "bands are whole multiples of 256 bytes: the payload keeps hipMalloc's alignment"
        self.pattern, self.nbytes = int(pattern), int(nbytes)
        self.buffers = []
        self.checked = 0

    def shorten(self, buf: "DeviceBuffer", nbytes: int):
        """tell the guard that buf's payload is `nbytes` shorter than what was allocated: the back band then starts that much earlier (the
        positive control of the containment tests; the bytes given up already hold the pattern in a buffer nobody has written yet)"""
        assert buf._guard is self and 0 <= nbytes <= buf.nbytes
        buf._guard_payload = buf.nbytes - int(nbytes)

    def _band(self, buf, side):
        H = _native.hip()
        lo = buf._base if side == "front" else buf.ptr + buf._guard_payload
        n = buf.ptr - buf._base if side == "front" else (buf._base + buf._alloc) - lo
        got = np.empty(n, np.uint8)
        _chk(H.si_hip_memcpy_d2h(got.ctypes.data_as(C.c_void_p), lo, n, None), "d2h")
        _chk(H.si_hip_stream_sync(None), "sync")
        return got

    def check_buffer(self, buf: "DeviceBuffer"):
        if buf._guard_checked:
            return
        buf._guard_checked = True
        self.checked += 1
        _chk(_native.hip().si_hip_device_sync(), "device sync")
        for side in ("front", "back"):
            got = self._band(buf, side)
            bad = np.nonzero(got != self.pattern)[0]
            if bad.size:
                # offsets from the payload edge: the byte just before the payload is -1, the first byte behind it +0
                first, last = int(bad[0]), int(bad[-1])
                rel = (lambda o: o - got.size) if side == "front" else (lambda o: o)
                raise ContainmentError("%s band of buffer #%d (%s, %s, %d bytes) overwritten: %d bytes differ from 0x%02X, offsets %+d .. %+d from the "
                                       "payload's %s" % (side, buf._guard_id, buf._guard_site, buf._guard_role(), buf._guard_payload, bad.size,
                                                         self.pattern, rel(first), rel(last), "start" if side == "front" else "end"))
        if buf._guard_host is not None:
            ref = np.frombuffer(buf._guard_host, np.uint8)
            got = buf.to_numpy((ref.size,), np.uint8)
            bad = np.nonzero(got != ref)[0]
            if bad.size:
                raise ContainmentError("input buffer #%d (%s, %d bytes) was written: %d bytes differ, first at byte %d" % (
                    buf._guard_id, buf._guard_site, buf.nbytes, bad.size, int(bad[0])))

    def check(self):
        """compare every live buffer created under this guard (also done when the context exits)"""
        for b in self.buffers:
            if b.ptr:
                self.check_buffer(b)


@contextlib.contextmanager
def guard_bands(pattern: int = 0xFF, nbytes: int = 4096):
    """with hipops.guard_bands(0xFF) as g: ...  -- every DeviceBuffer created inside (not DeviceBuffer.view) is allocated with `nbytes` more on
    either side of its payload, the whole allocation pre-filled with the byte `pattern`; the payload starts 256-byte aligned as without the guard
    and the back band starts at the payload's last byte + 1.  When a buffer is freed and when the block ends both bands are read back and
    compared with the pattern, and a buffer uploaded as an input (from_numpy) is compared with what was uploaded: ContainmentError names the
    buffer, the side and the offsets.  The bands are part of the test's own allocation: an overrun is observed, never provoked or trapped."""
    global _GUARD
    assert _GUARD is None, "guard_bands does not nest"
    g = _GUARD = GuardBands(pattern, nbytes)
    try:
        yield g
        g.check()
    finally:
        _GUARD = None
        for b in g.buffers:
            b._guard_checked = True
            b.free()
        g.buffers = []


class DeviceBuffer:
    """HBM allocation owned by Python (hipMalloc / hipFree through the C-ABI)."""

    def __init__(self, nbytes: int):
        self.nbytes = int(nbytes)
        g = _GUARD
        pad = g.nbytes if g is not None else 0
        self._alloc = max(self.nbytes + 2 * pad, 16)
        p = C.c_void_p()
        _chk(_native.hip().si_hip_malloc(C.byref(p), self._alloc), "si_hip_malloc")
        self._base = p.value
        self.ptr = self._base + pad
        self._guard = g
        if g is not None:
            self._guard_id, self._guard_site, self._guard_payload = len(g.buffers), _creation_site(), self.nbytes
            self._guard_host, self._guard_checked = None, False
            _chk(_native.hip().si_hip_memset_async(self._base, g.pattern, self._alloc, None), "memset")
            _chk(_native.hip().si_hip_stream_sync(None), "sync")
            g.buffers.append(self)

    def _guard_role(self):
        return "input" if self._guard_host is not None else "output / workspace"

    @classmethod
    def from_numpy(cls, a: np.ndarray, stream=None, out: bool = False) -> "DeviceBuffer":
        """out: the buffer is a destination pre-filled with `a` (a kernel may write it); else an input, which guard_bands() holds to its bytes"""
        a = np.ascontiguousarray(a)
        b = cls(a.nbytes)
        _chk(_native.hip().si_hip_memcpy_h2d(b.ptr, a.ctypes.data_as(C.c_void_p), a.nbytes, stream), "h2d")
        _chk(_native.hip().si_hip_stream_sync(stream), "sync")
        if b._guard is not None and not out:
            b._guard_host = a.tobytes()
        return b

    @classmethod
    def view(cls, ptr: int, nbytes: int) -> "DeviceBuffer":
        """Non-owning handle on device memory somebody else allocated (an engine output, a gathered buffer)."""
        b = cls.__new__(cls)
        b.nbytes, b.ptr, b._borrowed, b._guard = int(nbytes), int(ptr), True, None
        return b

    def to_numpy(self, shape, dtype=np.float32, stream=None) -> np.ndarray:
        out = np.empty(shape, dtype)
        assert out.nbytes <= max(self.nbytes, 16)
        _chk(_native.hip().si_hip_memcpy_d2h(out.ctypes.data_as(C.c_void_p), self.ptr, out.nbytes, stream), "d2h")
        _chk(_native.hip().si_hip_stream_sync(stream), "sync")
        return out

    def fill(self, byte: int = 0):
        _chk(_native.hip().si_hip_memset_async(self.ptr, byte, self.nbytes, None), "memset")
        _chk(_native.hip().si_hip_stream_sync(None), "sync")
        if getattr(self, "_guard", None) is not None:
            self._guard_host = None   # a buffer that is memset is a destination

    def free(self):
        if getattr(self, "ptr", None):
            if not getattr(self, "_borrowed", False):
                g = getattr(self, "_guard", None)
                if g is not None and not self._guard_checked:
                    g.check_buffer(self)
                _native.hip().si_hip_free(self._base)
            self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def sync():
    _chk(_native.hip().si_hip_device_sync(), "device sync")


def _f32(a) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=np.float32)


def _i4(shape: Sequence[int]):
    return (C.c_int * 4)(*[int(s) for s in shape])


def pad4(shape: Sequence[int]):
    shape = list(shape)
    if len(shape) >= 4:
        return [int(np.prod(shape[:len(shape) - 3]))] + shape[-3:]
    return [1] * (4 - len(shape)) + shape


def conv_out_hw(ih, iw, k, s, p, d):
    oh = (ih + 2 * p[0] - ((k[0] - 1) * d[0] + 1)) // s[0] + 1
    ow = (iw + 2 * p[1] - ((k[1] - 1) * d[1] + 1)) // s[1] + 1
    return oh, ow


# The strided-view hooks every wrapper below shares (the view contract: DESIGN.md "Views").  A tensor handed to a kernel as (ptr, ld, c) is the
# channel slice [c_off, c_off + c) of rows of ld elements; the wrappers build that row buffer, fill what is NOT the slice with a value or a
# ByteFill, hand the kernel the slice's pointer and -- full=True -- return the whole row buffer so that a test can look at the outside:
#   in_ld / in_c_off / in_fill      the input (the buffer is exactly pixels * in_ld elements: with in_c_off + ic == in_ld the slice ends at its end)
#   res_ld / res_c_off / res_fill   the fused residual
#   out_ld / out_c_off / out_fill   the destination, pre-filled with out_fill; full=True returns all out_ld channels
def _view_in(x, ld, c_off, fill):
    """(buffer, pointer to the slice) of x uploaded as channels [c_off, c_off + C) of rows of `ld` elements whose other channels hold `fill`"""
    c = x.shape[-1]
    ld = ld or c
    assert c_off >= 0 and c_off + c <= ld, (c_off, c, ld)
    if ld != c:
        w = _full(x.shape[:-1] + (ld,), x.dtype, fill)
        w[..., c_off:c_off + c] = x
        x = w
    b = DeviceBuffer.from_numpy(x)
    return b, b.ptr + x.itemsize * c_off


def _view_out(pixel_shape, c, ld, c_off, fill, dtype=np.float32):
    """(buffer, pointer to the slice) of a destination of rows of `ld` elements pre-filled with `fill`"""
    ld = ld or c
    assert c_off >= 0 and c_off + c <= ld, (c_off, c, ld)
    b = DeviceBuffer.from_numpy(_full(tuple(pixel_shape) + (ld,), dtype, fill), out=True)
    return b, b.ptr + np.dtype(dtype).itemsize * c_off


def _ret(y, c, c_off, full):
    """the wrappers' return value: the destination slice (as before), or with full=True the whole row buffer"""
    if full or y.shape[-1] == c:
        return y
    return y[..., c_off:c_off + c].copy()


def _run_desc_op(stem, d, x, out_pixel_shape, oc, in_ld, in_c_off, in_fill, out_ld, out_c_off, out_fill, full, operands=()):
    """what the descriptor wrappers share: si_hip_<stem>_f32 / _f16 (by x's dtype) with descriptor `d`, from the channel view of x to a fresh
    view of `out_pixel_shape` pixels of `oc` channels; records LAST_KERNEL_NAME["si_hip_<stem>"] for the two pointers.  operands: device
    pointers of further read-only operands, which the entry takes between x and the destination (the boxes of roi_align)"""
    H = _native.hip()
    half = x.dtype == np.float16
    name = "si_hip_%s_%s" % (stem, "f16" if half else "f32")
    out_pixel_shape = tuple(out_pixel_shape)
    (dx, px), (dy, py) = _view_in(x, in_ld, in_c_off, in_fill), _view_out(out_pixel_shape, oc, out_ld, out_c_off, out_fill, x.dtype)
    kernel_name = getattr(H, "si_hip_%s_kernel_name" % stem)
    mid = [C.c_void_p(int(p)) for p in operands]
    LAST_KERNEL_NAME["si_hip_" + stem] = kernel_name(C.byref(d), C.c_void_p(px), *mid, C.c_void_p(py), 1 if half else 0).decode()
    _chk(getattr(H, name)(C.byref(d), px, *mid, py, None), name)
    return _ret(dy.to_numpy(out_pixel_shape + (out_ld or oc,), x.dtype), oc, out_c_off, full)


def _desc_kernel_name(stem, d, half):
    """si_hip_<stem>_kernel_name for 16-byte aligned buffers"""
    return getattr(_native.hip(), "si_hip_%s_kernel_name" % stem)(C.byref(d), C.c_void_p(256), C.c_void_p(256), 1 if half else 0).decode()


def conv2d(x, w_oihw, bias=None, stride=(1, 1), padding=(0, 0), dilation=(1, 1), groups=1, act1="none",
           residual=None, act2="none", act_param=0.0, in_ld: Optional[int] = None, out_ld: Optional[int] = None,
           out_c_off: int = 0, in_fill=0.0, in_c_off: int = 0, res_ld: Optional[int] = None, res_c_off: int = 0, res_fill=0.0,
           out_fill=0.0, full: bool = False):
    """si_hip_conv2d_f32.  in_ld/out_ld > C exercise the strided (concat-slice) addressing: the input is
    embedded in / the output is written into a wider buffer and sliced back (the view hooks above)."""
    H = _native.hip()
    x, w_oihw = _f32(x), _f32(w_oihw)
    n, ih, iw, ic = x.shape
    oc, _, kh, kw = w_oihw.shape
    oh, ow = conv_out_hw(ih, iw, (kh, kw), stride, padding, dilation)
    in_ld = in_ld or ic
    out_ld = out_ld or oc
    d = SiConv2dDesc(n, ih, iw, ic, in_ld, oh, ow, oc, out_ld, kh, kw, stride[0], stride[1], dilation[0], dilation[1],
                     padding[0], padding[1], groups, 1 if bias is not None else 0, ACT[act1],
                     1 if residual is not None else 0, res_ld or oc, ACT[act2], float(act_param))
    packed = np.zeros(H.si_hip_conv2d_weight_elems(C.byref(d)), np.float32)
    _chk(H.si_hip_conv2d_pack_weight_host(C.byref(d), w_oihw.ctypes.data_as(C.c_void_p), packed.ctypes.data_as(C.c_void_p)),
         "pack weight")
    (dx, px), dw = _view_in(x, in_ld, in_c_off, in_fill), DeviceBuffer.from_numpy(packed)
    db = DeviceBuffer.from_numpy(_f32(bias)) if bias is not None else None
    dr, pr = _view_in(_f32(residual), res_ld, res_c_off, res_fill) if residual is not None else (None, None)
    dy, py = _view_out((n, oh, ow), oc, out_ld, out_c_off, out_fill)
    LAST_KERNEL_NAME["si_hip_conv2d_f32"] = H.si_hip_conv2d_kernel_name(C.byref(d), C.c_void_p(px)).decode()
    _chk(H.si_hip_conv2d_f32(C.byref(d), px, dw.ptr, db.ptr if db else None, pr, py, None), "si_hip_conv2d_f32")
    return _ret(dy.to_numpy((n, oh, ow, out_ld)), oc, out_c_off, full)


def conv_transpose_out_hw(ih, iw, k, s, p, op, d):
    """torch's output size of a transposed convolution"""
    return ((ih - 1) * s[0] - 2 * p[0] + d[0] * (k[0] - 1) + op[0] + 1,
            (iw - 1) * s[1] - 2 * p[1] + d[1] * (k[1] - 1) + op[1] + 1)


def conv_transpose2d_desc(x_shape, w_shape, bias=True, stride=(1, 1), padding=(0, 0), output_padding=(0, 0), dilation=(1, 1),
                          act1="none", act_param=0.0, in_ld=None, out_ld=None, groups=1):
    """SiConvTranspose2dDesc for an NHWC input of x_shape and a torch weight of w_shape [Cin][Cout/groups][kh][kw]"""
    n, ih, iw, ic = x_shape
    _, ocg, kh, kw = w_shape
    oc = ocg * groups
    oh, ow = conv_transpose_out_hw(ih, iw, (kh, kw), stride, padding, output_padding, dilation)
    return _native.SiConvTranspose2dDesc(n, ih, iw, ic, in_ld or ic, oh, ow, oc, out_ld or oc, kh, kw, stride[0], stride[1], padding[0],
                                         padding[1], output_padding[0], output_padding[1], dilation[0], dilation[1], groups,
                                         1 if bias else 0, ACT[act1], float(act_param))


def conv_transpose2d_pack(d, w_iohw) -> np.ndarray:
    """the kernel's weight image of a torch [Cin][Cout][kh][kw] weight (host only)"""
    H = _native.hip()
    w_iohw = _f32(w_iohw)
    packed = np.zeros(H.si_hip_conv_transpose2d_weight_elems(C.byref(d)), np.float32)
    _chk(H.si_hip_conv_transpose2d_pack_weight_host(C.byref(d), w_iohw.ctypes.data_as(C.c_void_p), packed.ctypes.data_as(C.c_void_p)),
         "pack transposed-conv weight")
    return packed


def conv_transpose2d(x_nhwc, w_iohw, bias=None, stride=(1, 1), padding=(0, 0), output_padding=(0, 0), dilation=(1, 1), act1="none",
                     act_param=0.0, in_ld: Optional[int] = None, out_ld: Optional[int] = None, out_c_off: int = 0, in_fill=0.0,
                     out_fill=0.0, full: bool = False, in_c_off: int = 0):
    """si_hip_conv_transpose2d_f32 (nn.ConvTranspose2d, groups = 1; w_iohw in torch's [Cin][Cout][kh][kw] layout).  As conv2d:
    in_ld > Cin embeds the input in a wider buffer whose other channels hold in_fill; out_ld > Cout writes channels
    [out_c_off, out_c_off + Cout) of a wider output buffer pre-filled with out_fill.  full=True returns that whole buffer."""
    H = _native.hip()
    x, w_iohw = _f32(x_nhwc), _f32(w_iohw)
    n, ih, iw, ic = x.shape
    assert w_iohw.shape[0] == ic, (x.shape, w_iohw.shape)
    oc = w_iohw.shape[1]
    in_ld = in_ld or ic
    out_ld = out_ld or oc
    assert out_c_off >= 0 and out_c_off + oc <= out_ld, (out_c_off, oc, out_ld)
    d = conv_transpose2d_desc(x.shape, w_iohw.shape, bias is not None, stride, padding, output_padding, dilation, act1, act_param, in_ld, out_ld)
    packed = conv_transpose2d_pack(d, w_iohw)
    oh, ow = d.oh, d.ow
    (dx, px), dw = _view_in(x, in_ld, in_c_off, in_fill), DeviceBuffer.from_numpy(packed)
    db = DeviceBuffer.from_numpy(_f32(bias)) if bias is not None else None
    dy = DeviceBuffer.from_numpy(_full((n, oh, ow, out_ld), np.float32, out_fill), out=True)
    _chk(H.si_hip_conv_transpose2d_f32(C.byref(d), px, dw.ptr, db.ptr if db else None, dy.ptr + 4 * out_c_off, None),
         "si_hip_conv_transpose2d_f32")
    y = dy.to_numpy((n, oh, ow, out_ld))
    if full or out_ld == oc:
        return y
    return y[..., out_c_off:out_c_off + oc].copy()


def conv_transpose2d_kernel_name(x_shape, w_shape, stride=(1, 1), padding=(0, 0), output_padding=(0, 0), dilation=(1, 1)) -> str:
    d = conv_transpose2d_desc(x_shape, w_shape, True, stride, padding, output_padding, dilation)
    return _native.hip().si_hip_conv_transpose2d_kernel_name(C.byref(d)).decode()


def deform_conv2d_desc(x_shape, off_shape, w_shape, mask=False, bias=True, stride=(1, 1), padding=(0, 0), dilation=(1, 1), groups=1, act1="none",
                       act_param=0.0, in_ld=None, off_ld=None, mask_ld=None, out_ld=None):
    """SiDeformConv2dDesc (include/si_deform.h) for an NHWC input of x_shape, an NHWC offset of off_shape [n, oh, ow, 2 og kh kw] and a torch
    weight of w_shape [Cout][Cin/groups][kh][kw]; the offset-group count is read off the offset's channels"""
    n, ih, iw, ic = x_shape
    oc, _, kh, kw = w_shape
    oh, ow = conv_out_hw(ih, iw, (kh, kw), stride, padding, dilation)
    off_c = int(off_shape[-1])
    og = off_c // (2 * kh * kw)
    return _native.SiDeformConv2dDesc(n, ih, iw, ic, in_ld or ic, oh, ow, oc, out_ld or oc, off_ld or off_c, (mask_ld or og * kh * kw) if mask else 0,
                                      kh, kw, stride[0], stride[1], padding[0], padding[1], dilation[0], dilation[1], groups, og,
                                      1 if mask else 0, 1 if bias else 0, ACT[act1], float(act_param))


def deform_conv2d_pack(d, w_oihw) -> np.ndarray:
    """the kernel's weight image of a torch [Cout][Cin/groups][kh][kw] weight (host only)"""
    H = _native.hip()
    w_oihw = _f32(w_oihw)
    packed = np.zeros(H.si_hip_deform_conv2d_weight_elems(C.byref(d)), np.float32)
    _chk(H.si_hip_deform_conv2d_pack_weight_host(C.byref(d), w_oihw.ctypes.data_as(C.c_void_p), packed.ctypes.data_as(C.c_void_p)),
         "pack deformable-conv weight")
    return packed


def deform_conv2d(x_nhwc, offset_nhwc, w_oihw, bias=None, mask_nhwc=None, stride=(1, 1), padding=(0, 0), dilation=(1, 1), groups=1, act1="none",
                  act_param=0.0, in_ld: Optional[int] = None, in_c_off: int = 0, in_fill=0.0, off_ld: Optional[int] = None, off_c_off: int = 0,
                  off_fill=0.0, mask_ld: Optional[int] = None, mask_c_off: int = 0, mask_fill=0.0, out_ld: Optional[int] = None, out_c_off: int = 0,
                  out_fill=0.0, full: bool = False):
    """si_hip_deform_conv2d_f32 (torchvision.ops.deform_conv2d; NHWC operands, w_oihw in torch's [Cout][Cin/groups][kh][kw] layout; without
    mask_nhwc DCNv1).  The view hooks are conv_transpose2d's, for all four views: x, offset and mask are each the channel slice
    [*_c_off, *_c_off + c) of rows of *_ld elements whose other channels hold *_fill; the destination is the slice [out_c_off, out_c_off + Cout)
    of rows of out_ld elements pre-filled with out_fill.  full=True returns the whole rows."""
    H = _native.hip()
    x, off, w_oihw = _f32(x_nhwc), _f32(offset_nhwc), _f32(w_oihw)
    mask = _f32(mask_nhwc) if mask_nhwc is not None else None
    oc = w_oihw.shape[0]
    d = deform_conv2d_desc(x.shape, off.shape, w_oihw.shape, mask is not None, bias is not None, stride, padding, dilation, groups, act1,
                           act_param, in_ld, off_ld, mask_ld, out_ld)
    assert off.shape[:3] == (d.n, d.oh, d.ow) and (mask is None or mask.shape[:3] == (d.n, d.oh, d.ow)), (x.shape, off.shape, (d.oh, d.ow))
    packed = deform_conv2d_pack(d, w_oihw)
    (dx, px), (do, po) = _view_in(x, in_ld, in_c_off, in_fill), _view_in(off, off_ld, off_c_off, off_fill)
    dm, pm = _view_in(mask, mask_ld, mask_c_off, mask_fill) if mask is not None else (None, None)
    dw = DeviceBuffer.from_numpy(packed)
    db = DeviceBuffer.from_numpy(_f32(bias)) if bias is not None else None
    dy, py = _view_out((d.n, d.oh, d.ow), oc, out_ld, out_c_off, out_fill)
    LAST_KERNEL_NAME["si_hip_deform_conv2d"] = H.si_hip_deform_conv2d_kernel_name(C.byref(d), C.c_void_p(px), C.c_void_p(po), C.c_void_p(pm) if pm else None,
                                                                                 C.c_void_p(py)).decode()
    _chk(H.si_hip_deform_conv2d_f32(C.byref(d), px, po, pm, dw.ptr, db.ptr if db else None, py, None), "si_hip_deform_conv2d_f32")
    return _ret(dy.to_numpy((d.n, d.oh, d.ow, out_ld or oc)), oc, out_c_off, full)


def deform_conv2d_kernel_name(x_shape, off_shape, w_shape, mask=False, stride=(1, 1), padding=(0, 0), dilation=(1, 1), groups=1, in_ld=None,
                              align=256) -> str:
    """the instantiation for dense operands (x rows of in_ld elements) whose x sits at address `align`; "none": a refused descriptor"""
    d = deform_conv2d_desc(x_shape, off_shape, w_shape, mask, True, stride, padding, dilation, groups, in_ld=in_ld)
    p = [C.c_void_p(int(align) + (1 << 32) * j) for j in range(4)]
    return _native.hip().si_hip_deform_conv2d_kernel_name(C.byref(d), p[0], p[1], p[2] if mask else None, p[3]).decode()


GRID_MODE = {"bilinear": 0, "nearest": 1, "bicubic": 2}
GRID_PADDING = {"zeros": 0, "border": 1, "reflection": 2}


def grid_sample_desc(x_shape, out_hw, mode="bilinear", padding_mode="zeros", align_corners=False, grid_strides=None, theta=False, in_ld=None,
                     out_ld=None, spatial_dims=2):
    """SiGridSampleDesc (include/si_grid.h) for an NHWC input of x_shape and an output of out_hw; grid_strides: the element strides
    (gs_n, gs_h, gs_w, gs_k) of the grid, torch's dense [n, ho, wo, 2] when None; theta: the coordinates come from a [n, 2, 3] theta"""
    n, h, w, c = x_shape
    ho, wo = out_hw
    gs = (0, 0, 0, 0) if theta else (tuple(grid_strides) if grid_strides is not None else (ho * wo * 2, wo * 2, 2, 1))
    return _native.SiGridSampleDesc(n, c, h, w, ho, wo, in_ld or 0, out_ld or 0, GRID_MODE[mode], GRID_PADDING[padding_mode], 1 if align_corners else 0,
                                    1 if theta else 0, spatial_dims, *[int(s) for s in gs])


def grid_sample(x, grid=None, mode="bilinear", padding_mode="zeros", align_corners=False, theta=None, out_hw=None, grid_strides=None,
                grid_off: int = 0, in_ld: Optional[int] = None, in_c_off: int = 0, in_fill=0.0, out_ld: Optional[int] = None, out_c_off: int = 0,
                out_fill=0.0, full: bool = False):
    """si_hip_grid_sample_f32 / _f16 (by x's dtype) on an NHWC x.  The coordinates come from `grid` -- an array of any shape that is uploaded as
    it lies in memory and addressed with the element strides grid_strides = (gs_n, gs_h, gs_w, gs_k) from element grid_off on; a [n, ho, wo, 2]
    array without strides is torch's dense grid -- or from theta= [n, 2, 3] with out_hw=(ho, wo) (F.affine_grid computed in the kernel).  The
    grid (or theta) is converted to x's storage type.  The view hooks of x and the destination are conv_transpose2d's."""
    H = _native.hip()
    x = _float_storage(x)
    half = x.dtype == np.float16
    n, h, w, c = x.shape
    assert (grid is None) != (theta is None), "give grid or theta"
    if theta is not None:
        src = np.ascontiguousarray(np.asarray(theta), dtype=x.dtype)
        assert src.shape == (n, 2, 3) and out_hw is not None, (src.shape, out_hw)
        ho, wo = out_hw
    else:
        src = np.ascontiguousarray(np.asarray(grid), dtype=x.dtype)
        if grid_strides is None:
            assert src.ndim == 4 and src.shape[0] == n and src.shape[3] == 2 and grid_off == 0, src.shape
            out_hw = src.shape[1:3]
        assert out_hw is not None, "a grid with explicit strides needs out_hw"
        ho, wo = out_hw
    d = grid_sample_desc(x.shape, (ho, wo), mode, padding_mode, align_corners, grid_strides, theta is not None, in_ld, out_ld)
    dx, px = _view_in(x, in_ld, in_c_off, in_fill)
    dg = DeviceBuffer.from_numpy(src)
    pg = dg.ptr + src.itemsize * int(grid_off)
    dy, py = _view_out((n, ho, wo), c, out_ld, out_c_off, out_fill, x.dtype)
    name = "si_hip_grid_sample_f16" if half else "si_hip_grid_sample_f32"
    LAST_KERNEL_NAME["si_hip_grid_sample"] = H.si_hip_grid_sample_kernel_name(C.byref(d), C.c_void_p(px), C.c_void_p(pg), C.c_void_p(py),
                                                                             1 if half else 0).decode()
    _chk(getattr(H, name)(C.byref(d), px, pg, py, None), name)
    return _ret(dy.to_numpy((n, ho, wo, out_ld or c), x.dtype), c, out_c_off, full)


def grid_sample_kernel_name(x_shape, out_hw, half=False, grid_strides=None, theta=False, in_ld=None, out_ld=None, align=256, grid_align=256) -> str:
    """the instantiation for operands far apart whose x and out sit at an address that is `align` modulo 256 and whose grid sits at `grid_align`;
    "none": a refused descriptor"""
    d = grid_sample_desc(x_shape, out_hw, grid_strides=grid_strides, theta=theta, in_ld=in_ld, out_ld=out_ld)
    p = [C.c_void_p(int(a) + (1 << 40) * (j + 1)) for j, a in enumerate((align, grid_align, align))]
    return _native.hip().si_hip_grid_sample_kernel_name(C.byref(d), p[0], p[1], p[2], 1 if half else 0).decode()


def affine_grid(theta, out_hw, align_corners=False, half=False, out_ld: Optional[int] = None, out_fill=0.0, full: bool = False):
    """si_hip_affine_grid_f32 / _f16: theta [n, 2, 3] -> the grid [n, H, W, 2] of F.affine_grid(theta, (n, C, H, W)).  The kernel writes this
    project's storage order of that rank-4 tensor, [n][W][2][H] with rows out_ld apart; the return value is the logical [n, H, W, 2] array
    (full=True: the stored rows, [n, W, 2, out_ld])"""
    H = _native.hip()
    dt = np.float16 if half else np.float32
    theta = np.ascontiguousarray(np.asarray(theta), dtype=dt)
    n = theta.shape[0]
    assert theta.shape == (n, 2, 3), theta.shape
    h, w = out_hw
    d = _native.SiAffineGridDesc(n, h, w, out_ld or 0, 1 if align_corners else 0)
    dt_, dy = DeviceBuffer.from_numpy(theta), DeviceBuffer.from_numpy(_full((n, w, 2, out_ld or h), dt, out_fill), out=True)
    name = "si_hip_affine_grid_f16" if half else "si_hip_affine_grid_f32"
    LAST_KERNEL_NAME["si_hip_affine_grid"] = H.si_hip_affine_grid_kernel_name(C.byref(d), C.c_void_p(dt_.ptr), C.c_void_p(dy.ptr), 1 if half else 0).decode()
    _chk(getattr(H, name)(C.byref(d), dt_.ptr, dy.ptr, None), name)
    y = dy.to_numpy((n, w, 2, out_ld or h), dt)
    return y if full else np.ascontiguousarray(y[..., :h].transpose(0, 3, 1, 2))


def roi_align_desc(x_shape, k, output_size, spatial_scale=1.0, sampling_ratio=-1, aligned=False, in_ld=None, out_ld=None, rois_ld=None):
    """SiRoiAlignDesc (include/si_roi.h) for an NHWC input of x_shape, k boxes and output_size = ph or (ph, pw)"""
    n, h, w, c = x_shape
    ph, pw = _pair(output_size)
    return _native.SiRoiAlignDesc(n, c, h, w, int(k), ph, pw, in_ld or 0, out_ld or 0, rois_ld or 0, int(sampling_ratio), 1 if aligned else 0,
                                  float(spatial_scale))


def roi_align(x, rois, output_size, spatial_scale=1.0, sampling_ratio=-1, aligned=False, rois_ld: Optional[int] = None, rois_fill=0.0,
              in_ld: Optional[int] = None, in_c_off: int = 0, in_fill=0.0, out_ld: Optional[int] = None, out_c_off: int = 0, out_fill=0.0,
              full: bool = False):
    """si_hip_roi_align_f32 / _f16 (by x's dtype) on an NHWC x [n, h, w, c] and boxes [k, 5] of (image index, x1, y1, x2, y2), which are
    uploaded as fp32 whatever x is, in rows of rois_ld floats whose other columns hold rois_fill.  Returns [k, ph, pw, c].  The view hooks of
    x and the destination are conv_transpose2d's."""
    x = _float_storage(x)
    rois = np.ascontiguousarray(np.asarray(rois), dtype=np.float32)
    assert rois.ndim == 2 and rois.shape[1] == 5, rois.shape
    k = rois.shape[0]
    if rois_ld and rois_ld != 5:
        rows = _full((k, rois_ld), np.float32, rois_fill)
        rows[:, :5] = rois
        rois = rows
    ph, pw = _pair(output_size)
    d = roi_align_desc(x.shape, k, (ph, pw), spatial_scale, sampling_ratio, aligned, in_ld, out_ld, rois_ld)
    dr = DeviceBuffer.from_numpy(rois)
    return _run_desc_op("roi_align", d, x, (k, ph, pw), x.shape[-1], in_ld, in_c_off, in_fill, out_ld, out_c_off, out_fill, full, operands=(dr.ptr,))


def roi_align_kernel_name(x_shape, k, output_size, half=False, sampling_ratio=-1, in_ld=None, out_ld=None, rois_ld=None, align=256) -> str:
    """the instantiation for operands far apart whose x and out sit at an address that is `align` modulo 256; "none": a refused descriptor"""
    d = roi_align_desc(x_shape, k, output_size, sampling_ratio=sampling_ratio, in_ld=in_ld, out_ld=out_ld, rois_ld=rois_ld)
    p = [C.c_void_p(int(a) + (1 << 40) * (j + 1)) for j, a in enumerate((align, 256, align))]
    return _native.hip().si_hip_roi_align_kernel_name(C.byref(d), p[0], p[1], p[2], 1 if half else 0).decode()


def _range_flag(d, want):
    """a zeroed device word handed to an f32_split launch as SiConv2dDesc::range_flag (the kernel writes 1 when an operand left fp16's range)"""
    if not want:
        return None
    f = DeviceBuffer.from_numpy(np.zeros(1, np.uint32))
    d.range_flag = f.ptr
    return f


def conv2d_split3(x, w_oihw, bias=None, stride=(1, 1), padding=(0, 0), act1="none", residual=None, act2="none", return_flag=False, in_ld=None,
                  in_fill=np.nan, in_c_off=0, res_ld=None, res_c_off=0, res_fill=0.0, out_ld=None, out_c_off=0, out_fill=0.0, full=False):
    """si_hip_conv2d_split3_f32: fp32 conv on the fp16 matrix cores by operand splitting (three fp16 MFMAs per product, fp32 accumulate).
    return_flag: also return the range-guard word (1: an operand overflowed fp16 on its way through the split).  in_ld: the input as a channel
    slice of a wider tensor (pixel stride in_ld > ic; what lies between is NaN)"""
    H = _native.hip()
    x, w_oihw = _f32(x), _f32(w_oihw)
    n, ih, iw, ic = x.shape
    oc, _, kh, kw = w_oihw.shape
    oh, ow = conv_out_hw(ih, iw, (kh, kw), stride, padding, (1, 1))
    d = SiConv2dDesc(n, ih, iw, ic, in_ld or ic, oh, ow, oc, out_ld or oc, kh, kw, stride[0], stride[1], 1, 1, padding[0], padding[1], 1,
                     1 if bias is not None else 0, ACT[act1], 1 if residual is not None else 0, res_ld or oc, ACT[act2], 0.0)
    if not H.si_hip_conv2d_split3_supported(C.byref(d)):
        raise HipError("si_hip_conv2d_split3_f32: unsupported shape")
    packed = np.zeros(H.si_hip_conv2d_split3_weight_elems(C.byref(d)), np.float16)
    _chk(H.si_hip_conv2d_split3_pack_weight_host(C.byref(d), w_oihw.ctypes.data_as(C.c_void_p), packed.ctypes.data_as(C.c_void_p)), "pack split3")
    (dx, px), dw = _view_in(x, in_ld, in_c_off, in_fill), DeviceBuffer.from_numpy(packed)
    db = DeviceBuffer.from_numpy(_f32(bias)) if bias is not None else None
    dr, pr = _view_in(_f32(residual), res_ld, res_c_off, res_fill) if residual is not None else (None, None)
    dy, py = _view_out((n, oh, ow), oc, out_ld, out_c_off, out_fill)
    flag = _range_flag(d, return_flag)
    _chk(H.si_hip_conv2d_split3_f32(C.byref(d), px, dw.ptr, db.ptr if db else None, pr, py, None), "si_hip_conv2d_split3_f32")
    y = _ret(dy.to_numpy((n, oh, ow, out_ld or oc)), oc, out_c_off, full)
    return (y, int(flag.to_numpy((1,), np.uint32)[0])) if return_flag else y


def conv2d_stem_split3(x, w_oihw, bias=None, stride=(2, 2), padding=(2, 2), act1="none", return_flag=False, in_ld=None, in_c_off=0, in_fill=0.0,
                       out_ld=None, out_c_off=0, out_fill=0.0, full=False):
    """si_hip_conv2d_stem_split3_f32: the RGB stem conv on the f32_split arithmetic (fp32 image in, fp32 activations out)"""
    H = _native.hip()
    x, w_oihw = _f32(x), _f32(w_oihw)
    n, ih, iw, ic = x.shape
    oc, _, kh, kw = w_oihw.shape
    oh, ow = conv_out_hw(ih, iw, (kh, kw), stride, padding, (1, 1))
    d = SiConv2dDesc(n, ih, iw, ic, in_ld or ic, oh, ow, oc, out_ld or oc, kh, kw, stride[0], stride[1], 1, 1, padding[0], padding[1], 1,
                     1 if bias is not None else 0, ACT[act1], 0, oc, ACT["none"], 0.0)
    if H.si_hip_conv2d_f16_supported(C.byref(d)) != 2:
        raise HipError("si_hip_conv2d_stem_split3_f32: not a stem shape")
    packed = np.zeros(H.si_hip_conv2d_stem_split3_weight_elems(C.byref(d)), np.float16)
    _chk(H.si_hip_conv2d_stem_split3_pack_weight_host(C.byref(d), w_oihw.ctypes.data_as(C.c_void_p), packed.ctypes.data_as(C.c_void_p)), "pack stem split3")
    (dx, px), dw = _view_in(x, in_ld, in_c_off, in_fill), DeviceBuffer.from_numpy(packed)
    db = DeviceBuffer.from_numpy(_f32(bias)) if bias is not None else None
    dy, py = _view_out((n, oh, ow), oc, out_ld, out_c_off, out_fill)
    flag = _range_flag(d, return_flag)
    _chk(H.si_hip_conv2d_stem_split3_f32(C.byref(d), px, dw.ptr, db.ptr if db else None, py, None), "si_hip_conv2d_stem_split3_f32")
    y = _ret(dy.to_numpy((n, oh, ow, out_ld or oc)), oc, out_c_off, full)
    return (y, int(flag.to_numpy((1,), np.uint32)[0])) if return_flag else y


def conv2d_wino23_split(x, w_oihw, bias=None, padding=(1, 1), act1="none", residual=None, act2="none", return_flag=False, in_ld=None, in_fill=0.0,
                        in_c_off=0, res_ld=None, res_c_off=0, res_fill=0.0, out_ld=None, out_c_off=0, out_fill=0.0, full=False):
    """si_hip_conv2d_wino23_split_f32: fused Winograd F(2,3) with the plane GEMMs on the fp16 matrix cores by operand splitting"""
    H = _native.hip()
    x, w_oihw = _f32(x), _f32(w_oihw)
    n, ih, iw, ic = x.shape
    oc = w_oihw.shape[0]
    oh, ow = conv_out_hw(ih, iw, (3, 3), (1, 1), padding, (1, 1))
    d = SiConv2dDesc(n, ih, iw, ic, in_ld or ic, oh, ow, oc, out_ld or oc, 3, 3, 1, 1, 1, 1, padding[0], padding[1], 1,
                     1 if bias is not None else 0, ACT[act1], 1 if residual is not None else 0, res_ld or oc, ACT[act2], 0.0)
    if not H.si_hip_conv2d_wino23_split_supported(C.byref(d)):
        raise HipError("si_hip_conv2d_wino23_split_f32: unsupported shape")
    packed = np.zeros(H.si_hip_conv2d_wino23_split_weight_elems(C.byref(d)), np.float16)
    _chk(H.si_hip_conv2d_wino23_split_pack_weight_host(C.byref(d), w_oihw.ctypes.data_as(C.c_void_p), packed.ctypes.data_as(C.c_void_p)), "pack wino split")
    (dx, px), dw = _view_in(x, in_ld, in_c_off, in_fill), DeviceBuffer.from_numpy(packed)
    db = DeviceBuffer.from_numpy(_f32(bias)) if bias is not None else None
    dr, pr = _view_in(_f32(residual), res_ld, res_c_off, res_fill) if residual is not None else (None, None)
    dy, py = _view_out((n, oh, ow), oc, out_ld, out_c_off, out_fill)
    flag = _range_flag(d, return_flag)
    _chk(H.si_hip_conv2d_wino23_split_f32(C.byref(d), px, dw.ptr, db.ptr if db else None, pr, py, None),
         "si_hip_conv2d_wino23_split_f32")
    y = _ret(dy.to_numpy((n, oh, ow, out_ld or oc)), oc, out_c_off, full)
    return (y, int(flag.to_numpy((1,), np.uint32)[0])) if return_flag else y


def _upcat(kind, low, skip, w_oihw, bias, scale, up_first, act1, split_oc, in_ld, in_c_off, in_fill, low_ld, low_c_off, out_ld, out_c_off,
           out2_ld, out2_c_off, out_fill, full):
    """the three dual-source entries (kind "f32" / "split3" / "f16") behind conv2d_upcat / conv2d_upcat_f16"""
    H = _native.hip()
    dt = np.float16 if kind == "f16" else np.float32
    low, skip, w_oihw = np.ascontiguousarray(low, dtype=dt), np.ascontiguousarray(skip, dtype=dt), _f32(w_oihw)
    n, oh, ow, cs = skip.shape
    _, lh, lw, cl = low.shape
    ic, oc = cl + cs, w_oihw.shape[0]
    assert w_oihw.shape[1] == ic and w_oihw.shape[2:] == (1, 1)
    ca = split_oc or oc
    d = SiConv2dDesc(n, oh, ow, ic, in_ld or ic, oh, ow, oc, out_ld or ca, 1, 1, 1, 1, 1, 1, 0, 0, 1, 1 if bias is not None else 0, ACT[act1], 0, oc, 0, 0.0)
    elems, pack, wdt = {"f32": (H.si_hip_conv2d_weight_elems, H.si_hip_conv2d_pack_weight_host, np.float32),
                        "split3": (H.si_hip_conv2d_split3_weight_elems, H.si_hip_conv2d_split3_pack_weight_host, np.float16),
                        "f16": (H.si_hip_conv2d_f16_weight_elems, H.si_hip_conv2d_f16_pack_weight_host, np.float16)}[kind]
    wp = np.zeros(elems(C.byref(d)), wdt)
    _chk(pack(C.byref(d), w_oihw.ctypes.data_as(C.c_void_p), wp.ctypes.data_as(C.c_void_p)), "pack " + kind)
    fname = {"f32": "si_hip_conv2d_upcat_f32", "split3": "si_hip_conv2d_split3_upcat_f32", "f16": "si_hip_conv2d_upcat_f16"}[kind]
    fn = getattr(H, fname)
    # the concat buffer: only the skip channels are ever written; the upsampled range is poisoned to prove nobody reads it
    cat = np.full((n, oh, ow, ic), np.nan, dt)
    c0 = 0 if up_first else cs
    cat[..., (cl if up_first else 0):(cl if up_first else 0) + cs] = skip
    (dcat, pcat), (dlow, plow), dw = _view_in(cat, in_ld, in_c_off, in_fill), _view_in(low, low_ld, low_c_off, in_fill), DeviceBuffer.from_numpy(wp)
    db = DeviceBuffer.from_numpy(_f32(bias)) if bias is not None else None
    up = _native.SiConv2dUpsampledSource(plow, lh, lw, cl, low_ld or cl, c0, np.float32(1.0) / np.float32(scale[0]), np.float32(1.0) / np.float32(scale[1]))
    dy, py = _view_out((n, oh, ow), ca, out_ld, out_c_off, out_fill, dt)
    if split_oc:
        dy2, py2 = _view_out((n, oh, ow), oc - split_oc, out2_ld, out2_c_off, out_fill, dt)
        _chk(fn(C.byref(d), pcat, C.byref(up), dw.ptr, db.ptr if db else None, py, split_oc, py2, out2_ld or oc - split_oc, None), fname)
        return (_ret(dy.to_numpy((n, oh, ow, out_ld or ca), dt), ca, out_c_off, full),
                _ret(dy2.to_numpy((n, oh, ow, out2_ld or oc - split_oc), dt), oc - split_oc, out2_c_off, full))
    _chk(fn(C.byref(d), pcat, C.byref(up), dw.ptr, db.ptr if db else None, py, 0, None, 0, None), fname)
    return _ret(dy.to_numpy((n, oh, ow, out_ld or oc), dt), oc, out_c_off, full)


def conv2d_upcat(low, skip, w_oihw, bias, scale=(2.0, 2.0), up_first=True, act1="none", split_oc=0, split3=False, in_ld=None, in_c_off=0, in_fill=0.0,
                 low_ld=None, low_c_off=0, out_ld=None, out_c_off=0, out2_ld=None, out2_c_off=0, out_fill=0.0, full=False):
    """si_hip_conv2d_upcat_f32: a 1x1 conv over cat([upsample(low), skip]) (or [skip, upsample(low)]) that reads `low` at the
    source pixel.  Returns y, or (y, y2) for the sibling-split form.  split3: the same on the f32_split arithmetic (si_hip_conv2d_split3_upcat_f32).
    in_ld / in_c_off: the concat buffer as a slice; low_ld / low_c_off: the low-resolution source as one (both gaps hold in_fill)."""
    return _upcat("split3" if split3 else "f32", low, skip, w_oihw, bias, scale, up_first, act1, split_oc, in_ld, in_c_off, in_fill, low_ld, low_c_off,
                  out_ld, out_c_off, out2_ld, out2_c_off, out_fill, full)


def conv2d_upcat_f16(low, skip, w_oihw, bias, scale=(2.0, 2.0), up_first=True, act1="none", split_oc=0, in_ld=None, in_c_off=0, in_fill=0.0,
                     low_ld=None, low_c_off=0, out_ld=None, out_c_off=0, out2_ld=None, out2_c_off=0, out_fill=0.0, full=False):
    """si_hip_conv2d_upcat_f16: conv2d_upcat with fp16 storage (half tensors in and out, fp32 bias)."""
    return _upcat("f16", low, skip, w_oihw, bias, scale, up_first, act1, split_oc, in_ld, in_c_off, in_fill, low_ld, low_c_off, out_ld, out_c_off,
                  out2_ld, out2_c_off, out_fill, full)


def conv2d_kernel_name(x_shape, w_shape, stride=(1, 1), padding=(0, 0), groups=1) -> str:
    """The kernel instantiation si_hip_conv2d_f32 picks for this shape with dense, 16-byte aligned tensors."""
    H = _native.hip()
    n, ih, iw, ic = x_shape
    oc, _, kh, kw = w_shape
    oh, ow = conv_out_hw(ih, iw, (kh, kw), stride, padding, (1, 1))
    d = SiConv2dDesc(n, ih, iw, ic, ic, oh, ow, oc, oc, kh, kw, stride[0], stride[1], 1, 1, padding[0], padding[1], groups, 1,
                     ACT["none"], 0, oc, ACT["none"], 0.0)
    return H.si_hip_conv2d_kernel_name(C.byref(d), C.c_void_p(4096)).decode()


def conv2d_winograd(x, w_oihw, bias=None, padding=(1, 1), act1="none", residual=None, act2="none", in_ld=None,
                    out_ld=None, out_c_off=0, tile=2, in_fill=0.0, in_c_off=0, res_ld=None, res_c_off=0, res_fill=0.0, out_fill=0.0, full=False):
    """si_hip_conv2d_wino23_f32 (tile=2, fused Winograd F(2,3)) or si_hip_conv2d_wino43_f32 (tile=4, F(4,3)); raises
    HipError for ineligible shapes."""
    H = _native.hip()
    fam = "wino23" if tile == 2 else "wino43"
    f_elig, f_elems = getattr(H, "si_hip_conv2d_%s_eligible" % fam), getattr(H, "si_hip_conv2d_%s_weight_elems" % fam)
    f_pack, f_run = getattr(H, "si_hip_conv2d_%s_pack_weight_host" % fam), getattr(H, "si_hip_conv2d_%s_f32" % fam)
    x, w_oihw = _f32(x), _f32(w_oihw)
    n, ih, iw, ic = x.shape
    oc = w_oihw.shape[0]
    oh, ow = ih + 2 * padding[0] - 2, iw + 2 * padding[1] - 2
    in_ld = in_ld or ic
    out_ld = out_ld or oc
    d = SiConv2dDesc(n, ih, iw, ic, in_ld, oh, ow, oc, out_ld, 3, 3, 1, 1, 1, 1, padding[0], padding[1], 1,
                     1 if bias is not None else 0, ACT[act1], 1 if residual is not None else 0, res_ld or oc, ACT[act2], 0.0)
    if not f_elig(C.byref(d)):
        raise HipError("shape not eligible for Winograd")
    u = np.zeros(f_elems(C.byref(d)), np.float32)
    _chk(f_pack(C.byref(d), w_oihw.ctypes.data_as(C.c_void_p), u.ctypes.data_as(C.c_void_p)), "wino pack")
    (dx, px), du = _view_in(x, in_ld, in_c_off, in_fill), DeviceBuffer.from_numpy(u)
    db = DeviceBuffer.from_numpy(_f32(bias)) if bias is not None else None
    dr, pr = _view_in(_f32(residual), res_ld, res_c_off, res_fill) if residual is not None else (None, None)
    dy, py = _view_out((n, oh, ow), oc, out_ld, out_c_off, out_fill)
    _chk(f_run(C.byref(d), px, du.ptr, db.ptr if db else None, pr, py, None), "si_hip_conv2d_%s_f32" % fam)
    return _ret(dy.to_numpy((n, oh, ow, out_ld)), oc, out_c_off, full)


def conv2d_split(x, w_a, b_a, w_b, b_b, act1="none", out2_ld=None, out2_c_off=0, in_ld=None, in_c_off=0, in_fill=0.0, out_ld=None, out_c_off=0,
                 out_fill=0.0, full=False):
    """si_hip_conv2d_split_f32: two 1x1 convs on the same input in one launch; returns (y_a, y_b)."""
    H = _native.hip()
    x, w_a, w_b = _f32(x), _f32(w_a), _f32(w_b)
    n, ih, iw, ic = x.shape
    oa, ob = w_a.shape[0], w_b.shape[0]
    out2_ld = out2_ld or ob

    def packed(w):
        d = SiConv2dDesc(n, ih, iw, ic, ic, ih, iw, w.shape[0], w.shape[0], 1, 1, 1, 1, 1, 1, 0, 0, 1, 1, 0, 0, 0, 0, 0.0)
        buf = np.zeros(H.si_hip_conv2d_weight_elems(C.byref(d)), np.float32)
        _chk(H.si_hip_conv2d_pack_weight_host(C.byref(d), w.ctypes.data_as(C.c_void_p), buf.ctypes.data_as(C.c_void_p)), "pack")
        return buf

    wcat = np.concatenate([packed(w_a), packed(w_b)])
    bcat = np.concatenate([_f32(b_a), _f32(b_b)])
    out_ld = out_ld or oa
    d = SiConv2dDesc(n, ih, iw, ic, in_ld or ic, ih, iw, oa + ob, out_ld, 1, 1, 1, 1, 1, 1, 0, 0, 1, 1, ACT[act1], 0, 0, 0, 0.0)
    (dx, px), dw, db = _view_in(x, in_ld, in_c_off, in_fill), DeviceBuffer.from_numpy(wcat), DeviceBuffer.from_numpy(bcat)
    (dya, pa), (dyb, pb) = _view_out((n, ih, iw), oa, out_ld, out_c_off, out_fill), _view_out((n, ih, iw), ob, out2_ld, out2_c_off, out_fill)
    _chk(H.si_hip_conv2d_split_f32(C.byref(d), px, dw.ptr, db.ptr, pa, oa, pb, out2_ld, None), "si_hip_conv2d_split_f32")
    return (_ret(dya.to_numpy((n, ih, iw, out_ld)), oa, out_c_off, full),
            _ret(dyb.to_numpy((n, ih, iw, out2_ld)), ob, out2_c_off, full or out2_ld == ob))


def conv2d_split3_split(x, w_a, b_a, w_b, b_b, act1="none", out2_ld=None, out2_c_off=0, in_ld=None, in_c_off=0, in_fill=0.0, out_ld=None, out_c_off=0,
                        out_fill=0.0, full=False):
    """si_hip_conv2d_split3_split_f32: two sibling 1x1 convs as one launch on the f32_split arithmetic; returns (y_a, y_b)"""
    H = _native.hip()
    x, w_a, w_b = _f32(x), _f32(w_a), _f32(w_b)
    n, ih, iw, ic = x.shape
    oa, ob = w_a.shape[0], w_b.shape[0]
    out2_ld = out2_ld or ob
    wcat = _f32(np.concatenate([w_a, w_b], 0))
    bcat = np.concatenate([_f32(b_a), _f32(b_b)])
    out_ld = out_ld or oa
    d = SiConv2dDesc(n, ih, iw, ic, in_ld or ic, ih, iw, oa + ob, out_ld, 1, 1, 1, 1, 1, 1, 0, 0, 1, 1, ACT[act1], 0, 0, 0, 0.0)
    packed = np.zeros(H.si_hip_conv2d_split3_weight_elems(C.byref(d)), np.float16)
    _chk(H.si_hip_conv2d_split3_pack_weight_host(C.byref(d), wcat.ctypes.data_as(C.c_void_p), packed.ctypes.data_as(C.c_void_p)), "pack split3")
    (dx, px), dw, db = _view_in(x, in_ld, in_c_off, in_fill), DeviceBuffer.from_numpy(packed), DeviceBuffer.from_numpy(bcat)
    (dya, pa), (dyb, pb) = _view_out((n, ih, iw), oa, out_ld, out_c_off, out_fill), _view_out((n, ih, iw), ob, out2_ld, out2_c_off, out_fill)
    _chk(H.si_hip_conv2d_split3_split_f32(C.byref(d), px, dw.ptr, db.ptr, pa, oa, pb, out2_ld, None), "si_hip_conv2d_split3_split_f32")
    return (_ret(dya.to_numpy((n, ih, iw, out_ld)), oa, out_c_off, full),
            _ret(dyb.to_numpy((n, ih, iw, out2_ld)), ob, out2_c_off, full or out2_ld == ob))


def linear(x, w, b=None):
    H = _native.hip()
    x, w = _f32(x), _f32(w)
    dx, dw = DeviceBuffer.from_numpy(x), DeviceBuffer.from_numpy(w)
    db = DeviceBuffer.from_numpy(_f32(b)) if b is not None else None
    dy = DeviceBuffer(x.shape[0] * w.shape[0] * 4)
    _chk(H.si_hip_linear_f32(dx.ptr, x.shape[0], x.shape[1], dw.ptr, db.ptr if db else None, w.shape[0], dy.ptr, None),
         "si_hip_linear_f32")
    return dy.to_numpy((x.shape[0], w.shape[0]))


def maxpool2d(x, k, s, p, d=(1, 1), in_ld=None, in_c_off=0, in_fill=0.0, out_ld=None, out_c_off=0, out_fill=0.0, full=False):
    H = _native.hip()
    x = _f32(x)
    n, ih, iw, c = x.shape
    oh, ow = conv_out_hw(ih, iw, k, s, p, d)
    desc = SiPool2dDesc(n, ih, iw, c, in_ld or c, oh, ow, out_ld or c, k[0], k[1], s[0], s[1], d[0], d[1], p[0], p[1])
    (dx, px), (dy, py) = _view_in(x, in_ld, in_c_off, in_fill), _view_out((n, oh, ow), c, out_ld, out_c_off, out_fill)
    _chk(H.si_hip_maxpool2d_f32(C.byref(desc), px, py, None), "si_hip_maxpool2d_f32")
    return _ret(dy.to_numpy((n, oh, ow, out_ld or c)), c, out_c_off, full)


def maxpool5_chain3(x, half=False, out_ld=None, out_c_off=(0, 0, 0), in_ld=None, in_c_off=0, in_fill=0.0, out_fill=0.0, full=False):
    """si_hip_maxpool5_chain3_{f32,f16}: the three chained 5x5 s1 p2 pools of SPPF; the outputs may be channel slices of
    wider rows (out_ld elements per pixel, starting at out_c_off[k]), as the concat aliasing hands them over."""
    H = _native.hip()
    x = _f16(x) if half else _f32(x)
    n, h, w, c = x.shape
    esz = 2 if half else 4
    ld = out_ld or c
    dt = np.float16 if half else np.float32
    dx, px = _view_in(x, in_ld, in_c_off, in_fill)
    outs = [_view_out((n, h, w), c, ld, off, out_fill, dt) for off in out_c_off]
    fn = H.si_hip_maxpool5_chain3_f16 if half else H.si_hip_maxpool5_chain3_f32
    _chk(fn(px, n, h, w, c, in_ld or c, outs[0][1], ld, outs[1][1], ld, outs[2][1], ld, None), "si_hip_maxpool5_chain3_f16" if half else "si_hip_maxpool5_chain3_f32")
    return [_ret(o.to_numpy((n, h, w, ld), dt), c, off, full) for (o, _), off in zip(outs, out_c_off)]


def adaptive_avgpool2d(x, out_hw, in_ld=None, in_c_off=0, in_fill=0.0, out_ld=None, out_c_off=0, out_fill=0.0, full=False):
    H = _native.hip()
    x = _f32(x)
    n, ih, iw, c = x.shape
    (dx, px), (dy, py) = _view_in(x, in_ld, in_c_off, in_fill), _view_out((n, out_hw[0], out_hw[1]), c, out_ld, out_c_off, out_fill)
    _chk(H.si_hip_adaptive_avgpool2d_f32(px, n, ih, iw, c, in_ld or c, py, out_hw[0], out_hw[1], out_ld or c, None),
         "si_hip_adaptive_avgpool2d_f32")
    return _ret(dy.to_numpy((n, out_hw[0], out_hw[1], out_ld or c)), c, out_c_off, full)


def upsample_nearest(x, scale_h, scale_w, out_hw=None, in_ld=None, in_c_off=0, in_fill=0.0, out_ld=None, out_c_off=0, out_fill=0.0, full=False):
    H = _native.hip()
    x = _f32(x)
    n, ih, iw, c = x.shape
    oh, ow = out_hw if out_hw else (int(ih * scale_h), int(iw * scale_w))
    (dx, px), (dy, py) = _view_in(x, in_ld, in_c_off, in_fill), _view_out((n, oh, ow), c, out_ld, out_c_off, out_fill)
    _chk(H.si_hip_upsample_nearest_f32(px, n, ih, iw, c, in_ld or c, scale_h, scale_w, py, oh, ow, out_ld or c, None),
         "si_hip_upsample_nearest_f32")
    return _ret(dy.to_numpy((n, oh, ow, out_ld or c)), c, out_c_off, full)


UPSAMPLE_MODE = {"nearest": 0, "bilinear": 1}


def upsample_out_hw(ih, iw, scale):
    """torch's output size of a scale factor: floor((double)in * scale) per axis (si_upsample_out_size, host only)"""
    H = _native.hip()
    sh, sw = (scale, scale) if np.isscalar(scale) else scale
    oh, ow = H.si_upsample_out_size(ih, float(sh)), H.si_upsample_out_size(iw, float(sw))
    if oh <= 0 or ow <= 0:
        raise ValueError("upsample: scale factor %r on %dx%d" % (scale, ih, iw))
    return oh, ow


def upsample_step(mode, n_in, n_out, align_corners=False, scale=None) -> np.float32:
    """the float32 source step of one axis (si_upsample_step, host only); scale None: not given, or recompute_scale_factor=True"""
    st = C.c_float()
    rc = _native.hip().si_upsample_step(UPSAMPLE_MODE[mode], n_in, n_out, 1 if align_corners else 0, float(scale or 0.0), C.byref(st))
    if rc != 0:
        raise ValueError("si_upsample_step(%s, %d, %d, align_corners=%s, scale=%r): code %d" % (mode, n_in, n_out, align_corners, scale, rc))
    return np.float32(st.value)


def upsample_desc(x_shape, out_hw=None, scale=None, align_corners=False, mode="bilinear", in_ld=None, out_ld=None):
    """SiUpsampleDesc of an NHWC input: out_hw (size=) or scale (scale_factor=, a number or a pair), exactly one of them"""
    assert (out_hw is None) != (scale is None), "give out_hw or scale"
    n, ih, iw, c = x_shape
    if scale is not None:
        sh, sw = (scale, scale) if np.isscalar(scale) else scale
        oh, ow = upsample_out_hw(ih, iw, (sh, sw))
    else:
        sh = sw = None
        oh, ow = out_hw
    return _native.SiUpsampleDesc(n, ih, iw, c, in_ld or c, oh, ow, out_ld or c, 1 if align_corners else 0,
                                  upsample_step(mode, ih, oh, align_corners, sh), upsample_step(mode, iw, ow, align_corners, sw))


def _float_storage(x):
    x = np.asarray(x)
    return np.ascontiguousarray(x) if x.dtype == np.float16 else _f32(x)


def upsample_bilinear(x, out_hw=None, scale=None, align_corners=False, in_ld: Optional[int] = None, in_fill=0.0,
                      out_ld: Optional[int] = None, out_c_off: int = 0, out_fill=0.0, full: bool = False, in_c_off: int = 0):
    """si_hip_upsample_bilinear_f32 / _f16 (by the array's dtype) on an NHWC array; out_hw = torch's size=, scale = its
    scale_factor= (recompute_scale_factor=True is out_hw=upsample_out_hw(...)).  The strided-view hooks are conv_transpose2d's."""
    H = _native.hip()
    x = _float_storage(x)
    half = x.dtype == np.float16
    n, ih, iw, c = x.shape
    in_ld, out_ld = in_ld or c, out_ld or c
    assert out_c_off >= 0 and out_c_off + c <= out_ld, (out_c_off, c, out_ld)
    d = upsample_desc(x.shape, out_hw, scale, align_corners, "bilinear", in_ld, out_ld)
    dx, px = _view_in(x, in_ld, in_c_off, in_fill)
    dy = DeviceBuffer.from_numpy(_full((n, d.oh, d.ow, out_ld), x.dtype, out_fill), out=True)
    fn = H.si_hip_upsample_bilinear_f16 if half else H.si_hip_upsample_bilinear_f32
    LAST_KERNEL_NAME["si_hip_upsample_bilinear"] = H.si_hip_upsample_bilinear_kernel_name(
        C.byref(d), C.c_void_p(px), C.c_void_p(dy.ptr + x.itemsize * out_c_off), 1 if half else 0).decode()
    _chk(fn(C.byref(d), px, dy.ptr + x.itemsize * out_c_off, None), "si_hip_upsample_bilinear_f16" if half else "si_hip_upsample_bilinear_f32")
    y = dy.to_numpy((n, d.oh, d.ow, out_ld), x.dtype)
    if full or out_ld == c:
        return y
    return y[..., out_c_off:out_c_off + c].copy()


def upsample_bilinear_kernel_name(x_shape, out_hw=None, scale=None, half=False, in_ld=None, out_ld=None) -> str:
    """the instantiation for 16-byte aligned buffers of these shapes"""
    d = upsample_desc(x_shape, out_hw, scale, False, "bilinear", in_ld, out_ld)
    return _desc_kernel_name("upsample_bilinear", d, half)


def upsample_nearest_size(x, out_hw, in_ld: Optional[int] = None, in_fill=0.0, in_c_off=0, out_ld=None, out_c_off=0, out_fill=0.0, full=False):
    """si_hip_upsample_nearest_steps_f32 with the steps of size= (torch's nearest rule)"""
    H = _native.hip()
    x = _f32(x)
    n, ih, iw, c = x.shape
    in_ld = in_ld or c
    d = upsample_desc(x.shape, out_hw, None, False, "nearest", in_ld)
    (dx, px), (dy, py) = _view_in(x, in_ld, in_c_off, in_fill), _view_out((n, d.oh, d.ow), c, out_ld, out_c_off, out_fill)
    _chk(H.si_hip_upsample_nearest_steps_f32(px, n, ih, iw, c, in_ld, d.step_h, d.step_w, py, d.oh, d.ow, out_ld or c, None),
         "si_hip_upsample_nearest_steps_f32")
    return _ret(dy.to_numpy((n, d.oh, d.ow, out_ld or c)), c, out_c_off, full)


def segment_labels(logits, out_hw, align_corners=False, in_ld: Optional[int] = None, in_fill=0.0, in_c_off: int = 0):
    """si_hip_segment_labels_f32 / _f16: uint8 [N, oh, ow] argmax over classes of the bilinear upsample of NHWC logits (the
    upsampled logits are never written)"""
    H = _native.hip()
    x = _float_storage(logits)
    n, ih, iw, c = x.shape
    in_ld = in_ld or c
    d = upsample_desc(x.shape, out_hw, None, align_corners, "bilinear", in_ld, 1)
    dx, px = _view_in(x, in_ld, in_c_off, in_fill)
    dy = DeviceBuffer(n * d.oh * d.ow)
    fn = H.si_hip_segment_labels_f16 if x.dtype == np.float16 else H.si_hip_segment_labels_f32
    _chk(fn(C.byref(d), px, dy.ptr, None), "si_hip_segment_labels_f16" if x.dtype == np.float16 else "si_hip_segment_labels_f32")
    return dy.to_numpy((n, d.oh, d.ow), np.uint8)


def cat(xs, axis, out_fill=None):
    """out_fill: the destination is pre-filled with this value or ByteFill (an element no kernel wrote then shows as the fill)"""
    H = _native.hip()
    xs = [_f32(x) for x in xs]
    shp = list(xs[0].shape)
    shp[axis] = sum(x.shape[axis] for x in xs)
    dy = DeviceBuffer(int(np.prod(shp)) * 4) if out_fill is None else DeviceBuffer.from_numpy(_full(tuple(shp), np.float32, out_fill), out=True)
    off = 0
    for x in xs:
        dx = DeviceBuffer.from_numpy(x)
        if axis == 3:
            _chk(H.si_hip_copy_channels_f32(dx.ptr, x.size // x.shape[3], x.shape[3], x.shape[3], dy.ptr + 4 * off,
                                            shp[3], None), "si_hip_copy_channels_f32")
        else:
            _chk(H.si_hip_cat_axis_f32(dx.ptr, _i4(x.shape), dy.ptr, _i4(shp), axis, off, None), "si_hip_cat_axis_f32")
        off += x.shape[axis]
        sync()
    return dy.to_numpy(shp)


def copy_channels(x, in_ld=None, in_c_off=0, in_fill=0.0, out_ld=None, out_c_off=0, out_fill=0.0, full=False):
    """si_hip_copy_channels_f32 on its own: the channels of x into channels [out_c_off, out_c_off + C) of rows of out_ld elements (one operand of
    a channel concat)"""
    H = _native.hip()
    x = _f32(x)
    c = x.shape[-1]
    (dx, px), (dy, py) = _view_in(x, in_ld, in_c_off, in_fill), _view_out(x.shape[:-1], c, out_ld, out_c_off, out_fill)
    _chk(H.si_hip_copy_channels_f32(px, x.size // c, c, in_ld or c, py, out_ld or c, None), "si_hip_copy_channels_f32")
    return _ret(dy.to_numpy(x.shape[:-1] + (out_ld or c,)), c, out_c_off, full)


def binary_op(op, a, b, out_shape=None, in_ld=None, in_c_off=0, in_fill=0.0, b_ld=None, b_c_off=0, out_ld=None, out_c_off=0, out_fill=0.0, full=False):
    """si_hip_binary_f32; in_ld / in_c_off are a's view, b_ld / b_c_off b's (both gaps hold in_fill); full=True returns the rank-4 row buffer"""
    H = _native.hip()
    a, b = _f32(a), _f32(b)
    a4, b4 = pad4(a.shape), pad4(b.shape)
    o4 = pad4(out_shape) if out_shape is not None else [max(x, y) for x, y in zip(a4, b4)]
    (da, pa), (db_, pb) = _view_in(a.reshape(a4), in_ld, in_c_off, in_fill), _view_in(b.reshape(b4), b_ld, b_c_off, in_fill)
    dy, py = _view_out(o4[:3], o4[3], out_ld, out_c_off, out_fill)
    _chk(H.si_hip_binary_f32(op, pa, _i4(a4), in_ld or a4[3], pb, _i4(b4), b_ld or b4[3], py, _i4(o4), out_ld or o4[3], None),
         "si_hip_binary_f32")
    y = dy.to_numpy(o4[:3] + [out_ld or o4[3]])
    if full:
        return y
    return _ret(y, o4[3], out_c_off, False).reshape(out_shape if out_shape is not None else o4)


def binary_const_desc(x_shape, ops, const_shapes, in_ld=None, out_ld=None, grid_cap=0):
    """SiBinaryDesc (include/si_binary.h) of a rank-4 x in storage order and one or two dense constants of rank-4 shapes that broadcast to it
    (a dimension is x's or 1): the strides of a dense array, 0 where the constant is broadcast"""
    d4 = [int(v) for v in x_shape]
    assert len(d4) == 4 and 1 <= len(ops) <= 2 and len(ops) == len(const_shapes)
    strides = []
    for cs in const_shapes:
        cs = [int(v) for v in cs]
        assert len(cs) == 4 and all(c == x or c == 1 for c, x in zip(cs, d4)), (cs, d4)
        dense = [cs[1] * cs[2] * cs[3], cs[2] * cs[3], cs[3], 1]
        strides.append([0 if c == 1 else s for c, s in zip(cs, dense)])
    strides.append([0, 0, 0, 0])
    ops = [int(o) for o in ops] + [0]
    I4, I2 = C.c_int * 4, C.c_int * 2
    return _native.SiBinaryDesc(I4(*d4), in_ld or d4[3], out_ld or d4[3], len(const_shapes), I2(*ops[:2]), I4(*strides[0]), I4(*strides[1]),
                                int(grid_cap))


def binary_const(x, ops, consts, c_off=0, grid_cap=0, in_ld=None, in_c_off=0, in_fill=0.0, out_ld=None, out_c_off=0, out_fill=0.0, full=False):
    """si_hip_binary_const_f32 / _f16 (by x's dtype): out = ops[1](ops[0](x, consts[0]), consts[1]) with the BinaryOp codes (7 / 8 / 9 / 11 put
    the constant first).  consts: arrays that broadcast to the rank-4 x, uploaded dense behind c_off spare elements (c_off = 1: a pointer that
    is not 16-byte aligned).  The view hooks are the common ones."""
    x = _float_storage(x)
    assert x.ndim == 4
    consts = [np.ascontiguousarray(c, dtype=x.dtype) for c in consts]
    d = binary_const_desc(x.shape, ops, [c.shape for c in consts], in_ld, out_ld, grid_cap)
    bufs = [DeviceBuffer.from_numpy(np.concatenate([np.zeros(c_off, x.dtype), c.reshape(-1)])) for c in consts]
    ptrs = [b.ptr + c_off * x.dtype.itemsize for b in bufs] + [0]
    return _run_desc_op("binary_const", d, x, x.shape[:3], x.shape[3], in_ld, in_c_off, in_fill, out_ld, out_c_off, out_fill, full,
                        operands=ptrs[:2])


def binary_const_kernel_name(x_shape, ops, const_shapes, half=False, in_ld=None, out_ld=None, grid_cap=0) -> str:
    """the instantiation for 16-byte aligned buffers of these shapes ("none": a descriptor the launch refuses)"""
    d = binary_const_desc(x_shape, ops, const_shapes, in_ld, out_ld, grid_cap)
    p = C.c_void_p(256)
    return _native.hip().si_hip_binary_const_kernel_name(C.byref(d), p, p, p, p, 1 if half else 0).decode()


def binary_scalar(op, x, scalar, in_ld=None, in_c_off=0, in_fill=0.0, out_ld=None, out_c_off=0, out_fill=0.0, full=False):
    """out = x (op) scalar -- BinaryOp's with_scalar form (op codes of include/si_hip.h; 7 / 8 / 9 / 11 put the scalar first)."""
    H = _native.hip()
    x = _f32(x)
    c = x.shape[-1]
    (dx, px), (dy, py) = _view_in(x, in_ld, in_c_off, in_fill), _view_out(x.shape[:-1], c, out_ld, out_c_off, out_fill)
    _chk(H.si_hip_binary_scalar_f32(op, px, x.size // c, c, in_ld or c, float(scalar), py, out_ld or c, None), "si_hip_binary_scalar_f32")
    return _ret(dy.to_numpy(x.shape[:-1] + (out_ld or c,)), c, out_c_off, full)


def unary_op(op, x, in_ld=None, out_ld=None, in_c_off=0, in_fill=np.nan, out_c_off=0, out_fill=0.0, full=False):
    """out = f(x) -- UnaryOp codes 0..17 (include/si_hip.h); optional pixel strides exercise the strided form."""
    H = _native.hip()
    x = _f32(x)
    c = x.shape[-1]
    pixels = x.size // c
    ild, old = in_ld or c, out_ld or c
    (dx, px), (dy, py) = _view_in(x.reshape(pixels, c), ild, in_c_off, in_fill), _view_out((pixels,), c, old, out_c_off, out_fill, np.float32)
    _chk(H.si_hip_unary_f32(op, px, pixels, c, ild, py, old, None), "si_hip_unary_f32")
    if full:
        return dy.to_numpy((pixels, old), np.float32)
    return dy.to_numpy((pixels, old))[:, out_c_off:out_c_off + c].reshape(x.shape)


def unary_op_f16(op, x, in_ld=None, out_ld=None, in_c_off=0, in_fill=np.nan, out_c_off=0, out_fill=0.0, full=False):
    """si_hip_unary_f16: UnaryOp on fp16 tensors (the fp32 function on the widened value, one rounding)."""
    H = _native.hip()
    x = _f16(x)
    c = x.shape[-1]
    pixels = x.size // c
    ild, old = in_ld or c, out_ld or c
    (dx, px), (dy, py) = _view_in(x.reshape(pixels, c), ild, in_c_off, in_fill), _view_out((pixels,), c, old, out_c_off, out_fill, np.float16)
    _chk(H.si_hip_unary_f16(op, px, pixels, c, ild, py, old, None), "si_hip_unary_f16")
    if full:
        return dy.to_numpy((pixels, old), np.float16)
    return dy.to_numpy((pixels, old), np.float16)[:, out_c_off:out_c_off + c].reshape(x.shape)


def activation(kind, x, param=0.0, in_ld=None, in_c_off=0, in_fill=0.0, out_ld=None, out_c_off=0, out_fill=0.0, full=False):
    H = _native.hip()
    x = _f32(x)
    c = x.shape[-1]
    (dx, px), (dy, py) = _view_in(x, in_ld, in_c_off, in_fill), _view_out(x.shape[:-1], c, out_ld, out_c_off, out_fill)
    _chk(H.si_hip_activation_f32(ACT[kind], param, px, x.size // c, c, in_ld or c, py, out_ld or c, None), "si_hip_activation_f32")
    return _ret(dy.to_numpy(x.shape[:-1] + (out_ld or c,)), c, out_c_off, full)


def batchnorm2d(x, mean, var, gamma, beta, eps, in_ld=None, in_c_off=0, in_fill=0.0, out_ld=None, out_c_off=0, out_fill=0.0, full=False):
    H = _native.hip()
    x = _f32(x)
    c = x.shape[-1]
    bufs = [DeviceBuffer.from_numpy(_f32(v)) for v in (mean, var, gamma, beta)]
    (dx, px), (dy, py) = _view_in(x, in_ld, in_c_off, in_fill), _view_out(x.shape[:-1], c, out_ld, out_c_off, out_fill)
    _chk(H.si_hip_batchnorm2d_f32(px, x.size // c, c, in_ld or c, bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, bufs[3].ptr, eps,
                                  py, out_ld or c, None), "si_hip_batchnorm2d_f32")
    return _ret(dy.to_numpy(x.shape[:-1] + (out_ld or c,)), c, out_c_off, full)


def group_norm_desc(x_shape, groups, eps=1e-5, affine=False, act1="none", act_param=0.0, in_ld=None, out_ld=None):
    """SiGroupNormDesc (include/si_norm.h) of an NHWC input"""
    n, h, w, c = x_shape
    return _native.SiGroupNormDesc(n, h, w, c, int(groups), in_ld or c, out_ld or c, float(eps), 1 if affine else 0, ACT[act1], float(act_param))


def group_norm(x, groups, gamma=None, beta=None, eps=1e-5, act1="none", act_param=0.0, half=False, in_ld=None, in_c_off=0, in_fill=0.0,
               out_ld=None, out_c_off=0, out_fill=0.0, full=False, workspace=True):
    """si_hip_groupnorm_f32 / _f16 (half=True, or an fp16 array) on an NHWC array: nn.GroupNorm(groups, C) in eval mode, nn.InstanceNorm2d
    with groups = C.  gamma / beta: both or neither.  The view hooks are the common ones; the workspace of the two-launch form is a
    DeviceBuffer of its own (guard_bands sees it); workspace=False hands the kernel a null workspace (the refusal test)."""
    H = _native.hip()
    x = np.asarray(x)
    half = bool(half) or x.dtype == np.float16
    x = _f16(x) if half else _f32(x)
    n, h, w, c = x.shape
    assert (gamma is None) == (beta is None), "gamma and beta: both or neither"
    d = group_norm_desc(x.shape, groups, eps, gamma is not None, act1, act_param, in_ld, out_ld)
    dg = DeviceBuffer.from_numpy(_f32(gamma)) if gamma is not None else None
    db = DeviceBuffer.from_numpy(_f32(beta)) if beta is not None else None
    (dx, px), (dy, py) = _view_in(x, in_ld, in_c_off, in_fill), _view_out(x.shape[:-1], c, out_ld, out_c_off, out_fill, x.dtype)
    nbytes = H.si_hip_groupnorm_workspace_bytes(C.byref(d))
    dw = DeviceBuffer(nbytes) if (nbytes and workspace) else None
    LAST_KERNEL_NAME["si_hip_groupnorm"] = H.si_hip_groupnorm_kernel_name(C.byref(d), C.c_void_p(px), C.c_void_p(py), 1 if half else 0).decode()
    fn, name = (H.si_hip_groupnorm_f16, "si_hip_groupnorm_f16") if half else (H.si_hip_groupnorm_f32, "si_hip_groupnorm_f32")
    _chk(fn(C.byref(d), px, dg.ptr if dg else None, db.ptr if db else None, py, dw.ptr if dw else None, None), name)
    return _ret(dy.to_numpy(x.shape[:-1] + (out_ld or c,), x.dtype), c, out_c_off, full)


def group_norm_kernel_name(x_shape, groups, half=False, in_ld=None, out_ld=None) -> str:
    """the kernel(s) for 16-byte aligned buffers of these shapes"""
    d = group_norm_desc(x_shape, groups, in_ld=in_ld, out_ld=out_ld)
    return _desc_kernel_name("groupnorm", d, half)


def group_norm_workspace_bytes(x_shape, groups) -> int:
    d = group_norm_desc(x_shape, groups)
    return int(_native.hip().si_hip_groupnorm_workspace_bytes(C.byref(d)))


PAD_MODE = {"constant": 0, "reflect": 1, "replicate": 2, "circular": 3}


def pad2d_desc(x_shape, pads, mode="constant", value=0.0, in_ld=None, out_ld=None):
    """SiPad2dDesc (include/si_pad.h) of an NHWC input; pads = (left, right, top, bottom) as torch orders them, negative: crop"""
    n, ih, iw, c = x_shape
    pl, pr, pt, pb = (int(p) for p in pads)
    return _native.SiPad2dDesc(n, ih, iw, c, in_ld or c, ih + pt + pb, iw + pl + pr, out_ld or c, pl, pr, pt, pb, PAD_MODE[mode], float(value))


def pad2d(x, pads, mode="constant", value=0.0, in_ld=None, in_c_off=0, in_fill=0.0, out_ld=None, out_c_off=0, out_fill=0.0, full=False):
    """si_hip_pad2d_f32 / _f16 (by the array's dtype) on an NHWC array: torch.nn.functional.pad(x, (l, r, t, b), mode, value) on the last
    two dimensions of the NCHW tensor.  The array's bits travel as they are (a NaN payload, -0.0).  The view hooks are the common ones."""
    x = _float_storage(x)
    n, ih, iw, c = x.shape
    d = pad2d_desc(x.shape, pads, mode, value, in_ld, out_ld)
    if d.oh < 1 or d.ow < 1:
        raise HipError("si_hip_pad2d: pads %r leave no output for a %dx%d input" % (tuple(pads), ih, iw))
    return _run_desc_op("pad2d", d, x, (n, d.oh, d.ow), c, in_ld, in_c_off, in_fill, out_ld, out_c_off, out_fill, full)


def pad2d_kernel_name(x_shape, pads, mode="constant", half=False, in_ld=None, out_ld=None) -> str:
    """the instantiation for 16-byte aligned buffers of these shapes ("none": a descriptor the launch refuses)"""
    d = pad2d_desc(x_shape, pads, mode, 0.0, in_ld, out_ld)
    return _desc_kernel_name("pad2d", d, half)


def _pair(v):
    return (int(v), int(v)) if isinstance(v, (int, np.integer)) else (int(v[0]), int(v[1]))


def avgpool_out_size(i, k, s, p, ceil_mode=False):
    """torch's output size of one axis of an average pool (include/si_pool.h); 0: the window does not fit"""
    span = i + 2 * p - k
    if span < 0:
        return 0
    o = (-(-span // s) if ceil_mode else span // s) + 1
    if ceil_mode and (o - 1) * s >= i + p:
        o -= 1
    return o


def avgpool2d_desc(x_shape, k, s=None, p=0, ceil_mode=False, count_include_pad=True, divisor_override=None, in_ld=None, out_ld=None):
    """SiAvgPool2dDesc (include/si_pool.h) of an NHWC input; k, s, p: an int or an (h, w) pair, s=None: the kernel size (torch's default)"""
    n, ih, iw, c = x_shape
    (kh, kw), (ph, pw) = _pair(k), _pair(p)
    sh, sw = (kh, kw) if s is None else _pair(s)
    oh = avgpool_out_size(ih, kh, sh, ph, ceil_mode) if sh > 0 else 0
    ow = avgpool_out_size(iw, kw, sw, pw, ceil_mode) if sw > 0 else 0
    return _native.SiAvgPool2dDesc(n, ih, iw, c, in_ld or c, oh, ow, out_ld or c, kh, kw, sh, sw, ph, pw, 0, 1 if count_include_pad else 0,
                                   int(divisor_override or 0))


def adaptive_avgpool2d_desc(x_shape, out_hw, in_ld=None, out_ld=None):
    n, ih, iw, c = x_shape
    return _native.SiAvgPool2dDesc(n, ih, iw, c, in_ld or c, int(out_hw[0]), int(out_hw[1]), out_ld or c, 0, 0, 0, 0, 0, 0, 1, 0, 0)


def _avgpool2d_run(x, d, in_ld, in_c_off, in_fill, out_ld, out_c_off, out_fill, full):
    if d.oh < 1 or d.ow < 1:
        raise HipError("si_hip_avgpool2d: no output for a %dx%d input" % (x.shape[1], x.shape[2]))
    return _run_desc_op("avgpool2d", d, x, (x.shape[0], d.oh, d.ow), x.shape[3], in_ld, in_c_off, in_fill, out_ld, out_c_off, out_fill, full)


def avgpool2d(x, k, s=None, p=0, ceil_mode=False, count_include_pad=True, divisor_override=None, in_ld=None, in_c_off=0, in_fill=0.0,
              out_ld=None, out_c_off=0, out_fill=0.0, full=False):
    """si_hip_avgpool2d_f32 / _f16 (by the array's dtype) on an NHWC array: torch.nn.functional.avg_pool2d(x, k, s, p, ceil_mode,
    count_include_pad, divisor_override) of the NCHW tensor.  The view hooks are the common ones."""
    x = _float_storage(x)
    d = avgpool2d_desc(x.shape, k, s, p, ceil_mode, count_include_pad, divisor_override, in_ld, out_ld)
    return _avgpool2d_run(x, d, in_ld, in_c_off, in_fill, out_ld, out_c_off, out_fill, full)


def adaptive_avgpool2d_general(x, out_hw, in_ld=None, in_c_off=0, in_fill=0.0, out_ld=None, out_c_off=0, out_fill=0.0, full=False):
    """si_hip_avgpool2d_f32 / _f16 with adaptive = 1: torch.nn.functional.adaptive_avg_pool2d for any output size (the engine sends the
    non-divisible shapes here; adaptive_avgpool2d above keeps the divisible ones)"""
    x = _float_storage(x)
    d = adaptive_avgpool2d_desc(x.shape, out_hw, in_ld, out_ld)
    return _avgpool2d_run(x, d, in_ld, in_c_off, in_fill, out_ld, out_c_off, out_fill, full)


def avgpool2d_kernel_name(x_shape, k=None, s=None, p=0, ceil_mode=False, half=False, in_ld=None, out_ld=None, adaptive=None) -> str:
    """the instantiation for 16-byte aligned buffers of these shapes ("none": a descriptor the launch refuses); adaptive=(oh, ow): the
    adaptive windows instead of k / s / p"""
    d = adaptive_avgpool2d_desc(x_shape, adaptive, in_ld, out_ld) if adaptive is not None else avgpool2d_desc(x_shape, k, s, p, ceil_mode, True, None,
                                                                                                                 in_ld, out_ld)
    return _desc_kernel_name("avgpool2d", d, half)


def softmax_desc(x_shape, axis, log=False, in_ld=None, out_ld=None):
    """SiSoftmaxDesc (include/si_softmax.h) of an NHWC input; axis: the NHWC axis reduced over"""
    n, h, w, c = x_shape
    return _native.SiSoftmaxDesc(n, h, w, c, in_ld or c, out_ld or c, int(axis), int(log))


def softmax(x, axis, log=False, in_ld=None, in_c_off=0, in_fill=0.0, out_ld=None, out_c_off=0, out_fill=0.0, full=False):
    """si_hip_softmax_f32 / _f16 (by the array's dtype) on an NHWC array: torch's softmax / log_softmax (log=True) along the NHWC axis
    `axis` (0 n, 1 h, 2 w, 3 c; negative counts from the end).  The view hooks are the common ones."""
    x = _float_storage(x)
    assert x.ndim == 4, "NHWC (a rank-2 [N, F] array is [N, 1, 1, F])"
    d = softmax_desc(x.shape, axis + 4 if axis < 0 else axis, log, in_ld, out_ld)
    return _run_desc_op("softmax", d, x, x.shape[:-1], x.shape[3], in_ld, in_c_off, in_fill, out_ld, out_c_off, out_fill, full)


def softmax_kernel_name(x_shape, axis, half=False, in_ld=None, out_ld=None) -> str:
    """the instantiation for 16-byte aligned buffers of these shapes ("none": a descriptor the launch refuses)"""
    d = softmax_desc(x_shape, axis, False, in_ld, out_ld)
    return _desc_kernel_name("softmax", d, half)


def attention_desc(batch, heads, lq, lk, d, scale=None, batch_first=False, q_ld=None, k_ld=None, v_ld=None, out_ld=None):
    """SiAttentionDesc (include/si_attention.h) of token tensors [L, N, E] (seq-first) or [N, L, E] (batch_first) with E = heads * d, whose
    token rows are q_ld / k_ld / v_ld / out_ld elements apart (default E: dense).  scale defaults to 1 / sqrt(d) in float32."""
    e = int(heads) * int(d)

    def strides(length, ld):
        ld = int(ld or e)
        return (int(length) * ld, ld) if batch_first else (ld, int(batch) * ld)

    dsc = _native.SiAttentionDesc()
    dsc.batch, dsc.heads, dsc.lq, dsc.lk, dsc.d = int(batch), int(heads), int(lq), int(lk), int(d)
    (dsc.q_sb, dsc.q_ss), (dsc.k_sb, dsc.k_ss) = strides(lq, q_ld), strides(lk, k_ld)
    (dsc.v_sb, dsc.v_ss), (dsc.o_sb, dsc.o_ss) = strides(lk, v_ld), strides(lq, out_ld)
    dsc.scale = float(np.float32(1.0) / np.sqrt(np.float32(d))) if scale is None else float(scale)
    return dsc


def attention(q, k, v, heads, scale=None, batch_first=False, packed=False, in_ld=None, in_c_off=0, in_fill=0.0, out_ld=None, out_c_off=0,
              out_fill=0.0, full=False):
    """si_hip_attention_f32 / _f16 (by q's dtype): softmax(scale * q k^T) v per (batch item, head) on token arrays [L, N, E] (seq-first) or
    [N, L, E] (batch_first), E = heads * d; k and v share their length, which may differ from q's.  The view hooks are the common ones: every
    input is the column slice [in_c_off, in_c_off + E) of rows of in_ld elements, the rest holding in_fill; packed=True (lq == lk) makes the
    three inputs the neighbouring slices q | k | v, from in_c_off on, of ONE buffer of rows of in_ld (default 3 E) elements, as the layer's
    projection workspace is.  The destination is the slice [out_c_off, out_c_off + E) of rows of out_ld elements pre-filled with out_fill;
    full=True returns the whole rows."""
    H = _native.hip()
    q, k, v = _float_storage(q), _float_storage(np.asarray(k)), _float_storage(np.asarray(v))
    assert q.ndim == k.ndim == v.ndim == 3 and q.dtype == k.dtype == v.dtype and k.shape == v.shape and q.shape[2] == k.shape[2], (q.shape, k.shape, v.shape)
    half = q.dtype == np.float16
    e = q.shape[2]
    assert e % heads == 0, (e, heads)
    batch, lq, lk = (q.shape[0], q.shape[1], k.shape[1]) if batch_first else (q.shape[1], q.shape[0], k.shape[0])
    assert (k.shape[0] if batch_first else k.shape[1]) == batch
    if packed:
        assert q.shape == k.shape, "one [rows, 3E] buffer: lq == lk"
        ld = in_ld or 3 * e
        assert in_c_off >= 0 and in_c_off + 3 * e <= ld, (in_c_off, e, ld)
        w = _full(q.shape[:-1] + (ld,), q.dtype, in_fill)
        for j, t in enumerate((q, k, v)):
            w[..., in_c_off + j * e:in_c_off + (j + 1) * e] = t
        dw = DeviceBuffer.from_numpy(w)
        pq, pk, pv = (dw.ptr + q.itemsize * (in_c_off + j * e) for j in range(3))
    else:
        ld = in_ld or e
        (dq, pq), (dk, pk), (dv, pv) = (_view_in(t, in_ld, in_c_off, in_fill) for t in (q, k, v))
    d = attention_desc(batch, heads, lq, lk, e // heads, scale, batch_first, ld, ld, ld, out_ld or e)
    dy, py = _view_out(q.shape[:-1], e, out_ld, out_c_off, out_fill, q.dtype)
    LAST_KERNEL_NAME["si_hip_attention"] = H.si_hip_attention_kernel_name(C.byref(d), C.c_void_p(pq), C.c_void_p(pk), C.c_void_p(pv), C.c_void_p(py),
                                                                         1 if half else 0).decode()
    name = "si_hip_attention_f16" if half else "si_hip_attention_f32"
    _chk(getattr(H, name)(C.byref(d), pq, pk, pv, py, None), name)
    return _ret(dy.to_numpy(q.shape[:-1] + (out_ld or e,), q.dtype), e, out_c_off, full)


def attention_kernel_name(d, half=False, heads=1, align=256) -> str:
    """the instantiation for dense seq-first tensors of head dim d at 16-byte aligned (align=256) addresses; "none": a refused descriptor"""
    dsc = attention_desc(1, heads, 1, 1, d)
    p = [C.c_void_p(int(align) + 65536 * j) for j in range(4)]
    return _native.hip().si_hip_attention_kernel_name(C.byref(dsc), p[0], p[1], p[2], p[3], 1 if half else 0).decode()


RNN_CELLS = {"lstm": 0, "gru": 1}
RNN_GATES = {"lstm": 4, "gru": 3}


def rnn_desc(cell, t, batch, input_size, hidden, dirs, batch_first=False, x_ld=None, g_ld=None, y_ld=None, step0=0):
    """SiRnnDesc (include/si_rnn.h) of x [T, N, I] (seq-first) or [N, T, I] (batch_first), the gate workspace [.., dirs * G * H] and y
    [.., dirs * H], whose rows are x_ld / g_ld / y_ld elements apart (default: dense).  cell: "lstm" / "gru" or the code"""
    code = RNN_CELLS[cell] if isinstance(cell, str) else int(cell)
    gates = 3 if code == 1 else 4

    def strides(ld):
        ld = int(ld)
        return (ld, int(t) * ld) if batch_first else (int(batch) * ld, ld)

    d = _native.SiRnnDesc()
    d.cell, d.t, d.batch, d.input, d.hidden, d.dirs, d.step0 = code, int(t), int(batch), int(input_size), int(hidden), int(dirs), int(step0)
    (d.x_st, d.x_sb), (d.g_st, d.g_sb) = strides(x_ld or input_size), strides(g_ld or dirs * gates * hidden)
    d.y_st, d.y_sb = strides(y_ld or dirs * hidden)
    return d


def rnn_pack_whh(d, w_hh, half=False) -> np.ndarray:
    """si_hip_rnn_pack_whh_f32 / _f16: w_hh fp32 [dirs, G * H, H] -> the step kernel's image (floats, or halves)"""
    H = _native.hip()
    w_hh = _f32(w_hh)
    nbytes = H.si_hip_rnn_workspace_bytes(C.byref(d), 2, 1 if half else 0)
    if nbytes == 0:
        raise HipError("no %s step kernel for this descriptor" % ("fp16" if half else "fp32"))
    image = np.zeros(nbytes // (2 if half else 4), np.float16 if half else np.float32)
    name = "si_hip_rnn_pack_whh_f16" if half else "si_hip_rnn_pack_whh_f32"
    _chk(getattr(H, name)(C.byref(d), w_hh.ctypes.data_as(C.c_void_p), image.ctypes.data_as(C.c_void_p)), name)
    return image


def rnn_layer(cell, gates, w_hh, b_hn=None, batch_first=False, want_state=False, input_size=8, g_ld=None, g_c_off=0, g_fill=0.0, out_ld=None,
              out_c_off=0, out_fill=0.0, full=False, c_fill=ByteFill(0xFF), step0=0, resume=None, return_c=False):
    """si_hip_rnn_layer_f32 / _f16 (by the gates' dtype): stages 2 and 3 of one layer on the projected gates [T, N, dirs * G * H] (seq-first) or
    [N, T, ..] (batch_first); w_hh fp32 [dirs, G * H, H]; b_hn fp32 [dirs, H] (GRU) or None.  The view hooks are the common ones, on the gates
    (g_*) and on y (out_*).  The c buffer starts as c_fill -- NaN bytes by default: the first step must not read it.  resume = (y, c): the
    dense y and the c buffer a call with step0 = 0 .. s - 1 left, to continue from step0 = s.  Returns y, with want_state (y, h_n, c_n) /
    (y, h_n); return_c appends the fp32 c buffer."""
    H = _native.hip()
    gates = _float_storage(gates)
    half = gates.dtype == np.float16
    w_hh = _f32(w_hh)
    dirs, gh, hidden = w_hh.shape
    ng = RNN_GATES[cell]
    assert gates.ndim == 3 and gh == ng * hidden and gates.shape[2] == dirs * gh, (gates.shape, w_hh.shape)
    batch, t = (gates.shape[0], gates.shape[1]) if batch_first else (gates.shape[1], gates.shape[0])
    yw = dirs * hidden
    d = rnn_desc(cell, t, batch, input_size, hidden, dirs, batch_first, None, g_ld or dirs * gh, out_ld or yw, step0)
    dimg = DeviceBuffer.from_numpy(rnn_pack_whh(d, w_hh, half))
    dg, pg = _view_in(gates, g_ld, g_c_off, g_fill)
    db = DeviceBuffer.from_numpy(_f32(b_hn)) if b_hn is not None else None
    if resume is not None:
        y0 = _full(gates.shape[:2] + (out_ld or yw,), gates.dtype, out_fill)
        y0[..., out_c_off:out_c_off + yw] = resume[0]
        dy = DeviceBuffer.from_numpy(y0, out=True)
        py = dy.ptr + gates.itemsize * out_c_off
    else:
        dy, py = _view_out(gates.shape[:2], yw, out_ld, out_c_off, out_fill, gates.dtype)
    lstm = cell == "lstm"
    dc = None
    if lstm:
        c0 = _f32(resume[1]) if resume is not None else _full((dirs, batch, hidden), np.float32, c_fill)
        dc = DeviceBuffer.from_numpy(c0, out=True)
    state_shape = (dirs, batch, hidden)
    dhn = DeviceBuffer.from_numpy(_full(state_shape, gates.dtype, out_fill), out=True) if want_state else None
    dcn = DeviceBuffer.from_numpy(_full(state_shape, gates.dtype, out_fill), out=True) if want_state and lstm else None
    LAST_KERNEL_NAME["si_hip_rnn"] = H.si_hip_rnn_kernel_name(C.byref(d), C.c_void_p(pg), C.c_void_p(py), 1 if half else 0).decode()
    name = "si_hip_rnn_layer_f16" if half else "si_hip_rnn_layer_f32"
    _chk(getattr(H, name)(C.byref(d), pg, dimg.ptr, db.ptr if db else None, py, dc.ptr if dc else None, dhn.ptr if dhn else None,
                          dcn.ptr if dcn else None, None), name)
    out = [_ret(dy.to_numpy(gates.shape[:2] + (out_ld or yw,), gates.dtype), yw, out_c_off, full)]
    if want_state:
        out.append(dhn.to_numpy(state_shape, gates.dtype))
        if lstm:
            out.append(dcn.to_numpy(state_shape, gates.dtype))
    if return_c:
        out.append(dc.to_numpy(state_shape, np.float32) if dc else None)
    return out[0] if len(out) == 1 else tuple(out)


def rnn_layer_f32(cell, gates, w_hh, b_hn=None, **kw):
    return rnn_layer(cell, np.asarray(gates, np.float32), w_hh, b_hn, **kw)


def rnn_layer_f16(cell, gates, w_hh, b_hn=None, **kw):
    return rnn_layer(cell, np.asarray(gates, np.float16), w_hh, b_hn, **kw)


def rnn_projection_bias(cell, b_ih, b_hh):
    """the bias of the input projection and b_hn, as include/si_rnn.h pins them: one fp32 sum on the host -- LSTM b_ih + b_hh; GRU b_ih + b_hh for r
    and z, b_ih alone for n, b_hn = b_hh's n rows"""
    b_ih, b_hh = _f32(b_ih), _f32(b_hh)
    if cell == "lstm":
        return b_ih + b_hh, None
    h = b_ih.size // 3
    return np.concatenate([b_ih[:2 * h] + b_hh[:2 * h], b_ih[2 * h:]]), b_hh[2 * h:].copy()


def _rnn(cell, x, weights, batch_first, want_state, views):
    x = _float_storage(x)
    half = x.dtype == np.float16
    states = []
    cur = x
    for l, per_dir in enumerate(weights):
        w_ih = np.concatenate([_f32(w[0]) for w in per_dir])
        w_hh = np.stack([_f32(w[1]) for w in per_dir])
        bias = b_hn = None
        if per_dir[0][2] is not None:
            parts = [rnn_projection_bias(cell, w[2], w[3]) for w in per_dir]
            bias = np.concatenate([p[0] for p in parts])
            b_hn = np.stack([p[1] for p in parts]) if cell == "gru" else None
        rows = cur.reshape(-1, 1, 1, cur.shape[2])
        conv = conv2d_f16 if half else conv2d
        gates = conv(rows, w_ih.reshape(w_ih.shape + (1, 1)), bias).reshape(cur.shape[:2] + (w_ih.shape[0],))
        last = l == len(weights) - 1
        res = rnn_layer(cell, gates, w_hh, b_hn, batch_first=batch_first, want_state=want_state, input_size=cur.shape[2], **(views if last else {}))
        cur = res[0] if want_state else res
        if want_state:
            states.append(res[1:])
    if not want_state:
        return cur
    return (cur,) + tuple(np.concatenate([s[j] for s in states]) for j in range(len(states[0])))


def lstm(x, weights, batch_first=False, want_state=False, **views):
    """torch.nn.LSTM in eval mode on a numpy array [T, N, I] (or [N, T, I]): per layer the input projection through si_hip_conv2d_f32 / _f16 and
    si_hip_rnn_layer_f32 / _f16 (by x's dtype).  weights[layer][direction] = (w_ih, w_hh, b_ih, b_hh), the biases None without bias.  The view
    hooks (out_ld, out_c_off, out_fill, full) apply to y of the last layer.  want_state: (y, h_n, c_n) with the states [layers * dirs, N, H]"""
    return _rnn("lstm", x, weights, batch_first, want_state, views)


def gru(x, weights, batch_first=False, want_state=False, **views):
    """torch.nn.GRU in eval mode, as lstm() above; want_state: (y, h_n)"""
    return _rnn("gru", x, weights, batch_first, want_state, views)


def conv1d_pads(k, padding, dilation=1, stride=1):
    """(left, right) zero pads of nn.Conv1d: an int pads both sides; 'valid' none; 'same' (stride 1) d (K - 1) in all, the odd one on the right"""
    if padding == "valid":
        return 0, 0
    if padding == "same":
        assert int(stride) == 1, "padding='same' needs stride 1"
        total = int(dilation) * (int(k) - 1)
        return total // 2, total - total // 2
    return int(padding), int(padding)


def conv1d_out_len(l, k, stride=1, padding=0, dilation=1):
    pl, pr = conv1d_pads(k, padding, dilation, stride)
    e = int(l) + pl + pr - int(dilation) * (int(k) - 1) - 1
    return e // int(stride) + 1 if e >= 0 else 0


def conv1d_desc(n, c, l, oc, k, stride=1, padding=0, dilation=1, groups=1, act="none", act_param=0.0, x_sn=None, x_sc=None, y_sn=None, y_sc=None,
                lo=None):
    """SiConv1dDesc (include/si_conv1d.h) of x [N, C, L] -> y [N, OC, Lo]; the strides default to dense tensors, lo to torch's formula"""
    d = _native.SiConv1dDesc()
    d.n, d.c, d.l, d.oc, d.k, d.stride, d.dilation, d.groups = int(n), int(c), int(l), int(oc), int(k), int(stride), int(dilation), int(groups)
    d.pad_left = conv1d_pads(k, padding, dilation, stride)[0]
    d.lo = int(lo) if lo is not None else conv1d_out_len(l, k, stride, padding, dilation)
    d.x_sc = int(x_sc) if x_sc is not None else d.l
    d.x_sn = int(x_sn) if x_sn is not None else d.c * d.x_sc
    d.y_sc = int(y_sc) if y_sc is not None else d.lo
    d.y_sn = int(y_sn) if y_sn is not None else d.oc * d.y_sc
    d.act = ACT[act] if isinstance(act, str) else int(act)
    d.act_param = float(act_param)
    return d


def conv1d_pack_weights(w, groups=1, half=False) -> np.ndarray:
    """si_hip_conv1d_pack_weights_f32 / _f16: torch's weight fp32 [OC, C / groups, K] -> the kernels' image (floats, or halves)"""
    H = _native.hip()
    w = _f32(w)
    oc, cg, k = w.shape
    d = conv1d_desc(1, cg * int(groups), 1, oc, k, groups=groups, lo=1)
    nbytes = H.si_hip_conv1d_weight_bytes(C.byref(d), 1 if half else 0)
    LAST_ENTRIES.append("si_hip_conv1d_weight_bytes")
    if nbytes == 0:
        raise HipError("no %s conv1d kernel for this filter" % ("fp16" if half else "fp32"))
    image = np.zeros(nbytes // (2 if half else 4), np.float16 if half else np.float32)
    name = "si_hip_conv1d_pack_weights_f16" if half else "si_hip_conv1d_pack_weights_f32"
    _chk(getattr(H, name)(C.byref(d), w.ctypes.data_as(C.c_void_p), image.ctypes.data_as(C.c_void_p)), name)
    return image


def conv1d(x, w, b=None, stride=1, padding=0, dilation=1, groups=1, act="none", act_param=0.0, in_c_total=None, in_c_off=0, in_ld=None,
           in_l_off=0, in_fill=0.0, out_c_total=None, out_c_off=0, out_ld=None, out_l_off=0, out_fill=0.0, full=False):
    """torch.nn.functional.conv1d (zero padding: an int, 'same' or 'valid') with a fused activation, through si_hip_conv1d_f32 / _f16 (by x's
    dtype).  x [N, C, L]; w fp32 [OC, C / groups, K]; b fp32 [OC] or None.  The view hooks make x channels [in_c_off, in_c_off + C) and
    positions [in_l_off, in_l_off + L) of a tensor [N, in_c_total, in_ld] whose other elements hold in_fill, and y the same kind of window of a
    tensor [N, out_c_total, out_ld] pre-filled with out_fill; full=True returns that whole tensor"""
    H = _native.hip()
    x = _float_storage(x)
    half = x.dtype == np.float16
    w = _f32(w)
    n, c, l = x.shape
    oc, cg, k = w.shape
    assert cg * int(groups) == c, (x.shape, w.shape, groups)
    lo = conv1d_out_len(l, k, stride, padding, dilation)
    ict, ild, oct_, old = int(in_c_total or c), int(in_ld or l), int(out_c_total or oc), int(out_ld or lo)
    assert 0 <= in_c_off and in_c_off + c <= ict and 0 <= in_l_off and in_l_off + l <= ild
    assert 0 <= out_c_off and out_c_off + oc <= oct_ and 0 <= out_l_off and out_l_off + lo <= old
    d = conv1d_desc(n, c, l, oc, k, stride, padding, dilation, groups, act, act_param, x_sn=ict * ild, x_sc=ild, y_sn=oct_ * old, y_sc=old)
    dimg = DeviceBuffer.from_numpy(conv1d_pack_weights(w, groups, half))
    xw = x
    if (ict, ild) != (c, l):
        xw = _full((n, ict, ild), x.dtype, in_fill)
        xw[:, in_c_off:in_c_off + c, in_l_off:in_l_off + l] = x
    dx = DeviceBuffer.from_numpy(xw)
    px = dx.ptr + x.itemsize * (in_c_off * ild + in_l_off)
    dy = DeviceBuffer.from_numpy(_full((n, oct_, old), x.dtype, out_fill), out=True)
    py = dy.ptr + x.itemsize * (out_c_off * old + out_l_off)
    db = DeviceBuffer.from_numpy(_f32(b)) if b is not None else None
    LAST_KERNEL_NAME["si_hip_conv1d"] = H.si_hip_conv1d_kernel_name(C.byref(d), C.c_void_p(px), C.c_void_p(py), 1 if half else 0).decode()
    name = "si_hip_conv1d_f16" if half else "si_hip_conv1d_f32"
    _chk(getattr(H, name)(C.byref(d), px, dimg.ptr, db.ptr if db else None, py, None), name)
    y = dy.to_numpy((n, oct_, old), x.dtype)
    if full:
        return y
    return np.ascontiguousarray(y[:, out_c_off:out_c_off + oc, out_l_off:out_l_off + lo])


def conv1d_kernel_name(n, c, l, oc, k, stride=1, padding=0, dilation=1, groups=1, half=False) -> str:
    """the instantiation for dense tensors at aligned addresses; "none": a refused descriptor"""
    d = conv1d_desc(n, c, l, oc, k, stride, padding, dilation, groups)
    return _native.hip().si_hip_conv1d_kernel_name(C.byref(d), C.c_void_p(1 << 24), C.c_void_p(1 << 30), 1 if half else 0).decode()


def xcorr_pads(kh, kw, padding, dilation=1, stride=1):
    """((top, bottom), (left, right)) zero pads of F.conv2d: an int or a pair pads both sides; 'valid' none; 'same' (stride 1) d (K - 1) per
    axis, the odd one on the far side"""
    (dh, dw), (sh, sw) = _pair(dilation), _pair(stride)
    if isinstance(padding, str):
        if padding == "valid":
            return (0, 0), (0, 0)
        assert padding == "same" and sh == 1 and sw == 1, "padding='same' needs stride 1"
        th, tw = dh * (int(kh) - 1), dw * (int(kw) - 1)
        return (th // 2, th - th // 2), (tw // 2, tw - tw // 2)
    ph, pw = _pair(padding)
    return (ph, ph), (pw, pw)


def xcorr_out_hw(h, w, kh, kw, stride=1, padding=0, dilation=1):
    (pt, pb), (pl, pr) = xcorr_pads(kh, kw, padding, dilation, stride)
    (sh, sw), (dh, dw) = _pair(stride), _pair(dilation)
    eh, ew = int(h) + pt + pb - dh * (int(kh) - 1) - 1, int(w) + pl + pr - dw * (int(kw) - 1) - 1
    return (eh // sh + 1 if eh >= 0 else 0), (ew // sw + 1 if ew >= 0 else 0)


def xcorr_desc(n, h, w, c, oc, kh, kw, stride=1, padding=0, dilation=1, groups=1, act="none", act_param=0.0, per_sample=False, ho=None, wo=None,
               **strides):
    """SiXcorrDesc (include/si_xcorr.h) of x [N, H, W, C] * w -> y [N, Ho, Wo, OC].  The strides default to dense NHWC tensors with the filter
    as stored: dense [OC][kh][kw][C]; depthwise [C][kh][kw][1] (the unfused addressing) or, per_sample, [N][kh][kw][C]"""
    d = _native.SiXcorrDesc()
    d.n, d.h, d.w, d.c, d.oc, d.kh, d.kw, d.groups = int(n), int(h), int(w), int(c), int(oc), int(kh), int(kw), int(groups)
    (d.stride_h, d.stride_w), (d.dilation_h, d.dilation_w) = _pair(stride), _pair(dilation)
    (d.pad_top, _), (d.pad_left, _) = xcorr_pads(kh, kw, padding, dilation, stride)
    oh, ow = xcorr_out_hw(h, w, kh, kw, stride, padding, dilation)
    d.ho, d.wo = int(ho) if ho is not None else oh, int(wo) if wo is not None else ow
    d.x_sp, d.x_sh, d.x_sn = d.c, d.w * d.c, d.h * d.w * d.c
    d.y_sp, d.y_sh, d.y_sn = d.oc, d.wo * d.oc, d.ho * d.wo * d.oc
    if per_sample or (int(groups) == 1 and not d.c == d.oc == 1):
        d.w_sc, d.w_sp, d.w_sh, d.w_sn = 1, d.c, d.kw * d.c, d.kh * d.kw * d.c
    else:
        d.w_sc, d.w_sp, d.w_sh, d.w_sn = d.kh * d.kw, 1, d.kw, 0
    for k, v in strides.items():
        assert k in ("x_sn", "x_sh", "x_sp", "w_sn", "w_sh", "w_sp", "w_sc", "y_sn", "y_sh", "y_sp"), k
        setattr(d, k, int(v))
    d.per_sample = 1 if per_sample else 0
    d.act = ACT[act] if isinstance(act, str) else int(act)
    d.act_param = float(act_param)
    return d


def _window(a, c_total, c_off, w_total, w_off, fill):
    """`a` [.., W, C] as the window [.., w_off : w_off + W, c_off : c_off + C] of a tensor [.., w_total, c_total] filled with `fill`:
    (the wide array, the element offset of the window's first element, the pixel stride, the row stride)"""
    wd, c = a.shape[-2], a.shape[-1]
    ct, wt = int(c_total or c), int(w_total or wd)
    assert 0 <= c_off and c_off + c <= ct and 0 <= w_off and w_off + wd <= wt
    wide = a
    if (ct, wt) != (c, wd):
        wide = _full(a.shape[:-2] + (wt, ct), a.dtype, fill)
        wide[..., w_off:w_off + wd, c_off:c_off + c] = a
    return wide, w_off * ct + c_off, ct, wt * ct


def xcorr(x, w, b=None, stride=1, padding=0, dilation=1, groups=1, act="none", act_param=0.0, per_sample=False,
          in_c_total=None, in_c_off=0, in_w_total=None, in_w_off=0, in_fill=0.0,
          w_c_total=None, w_c_off=0, w_w_total=None, w_w_off=0, w_fill=0.0,
          out_c_total=None, out_c_off=0, out_w_total=None, out_w_off=0, out_fill=0.0, full=False):
    """F.conv2d with a TENSOR filter and a fused activation through si_hip_xcorr_f32 / _f16 (by x's dtype).  NHWC arrays, the filter as the
    engine stores it: x [N, H, W, C]; w [OC, kh, kw, C] (groups == 1), [C, kh, kw, 1] (groups == C == OC) or, per_sample, [N, kh, kw, C]
    (filter n meets image n: the fused depthwise cross-correlation); b fp32 [OC] or None.  The view hooks make x, w and y windows
    [.., w_off : w_off + W, c_off : c_off + C] of tensors [.., w_total, c_total] whose other elements hold the fill (y: pre-filled with
    out_fill); full=True returns that whole tensor"""
    H = _native.hip()
    x = _float_storage(x)
    half = x.dtype == np.float16
    w = np.ascontiguousarray(w, dtype=x.dtype)
    n, h, wd, c = x.shape
    depthwise = per_sample or (int(groups) == c and w.shape[0] == c)
    if per_sample:
        assert w.shape[0] == n and w.shape[3] == c, (x.shape, w.shape)
        oc, groups = c, c
    else:
        oc = w.shape[0]
        assert w.shape[3] * int(groups) == c, (x.shape, w.shape, groups)
    kh, kw = w.shape[1], w.shape[2]
    ho, wo = xcorr_out_hw(h, wd, kh, kw, stride, padding, dilation)
    xw, x_off, x_sp, x_sh = _window(x, in_c_total, in_c_off, in_w_total, in_w_off, in_fill)
    ww, w_off, w_sp, w_sh = _window(w, w_c_total, w_c_off, w_w_total, w_w_off, w_fill)
    yw, y_off, y_sp, y_sh = _window(np.zeros((n, ho, wo, oc), x.dtype), out_c_total, out_c_off, out_w_total, out_w_off, 0.0)
    yw = _full(yw.shape, x.dtype, out_fill)
    if depthwise and not per_sample:
        wst = dict(w_sn=0, w_sc=kh * w_sh, w_sh=w_sh, w_sp=w_sp)      # a channel's filter is one "image" of the stored [C][kh][kw][1]
    else:
        wst = dict(w_sn=kh * w_sh, w_sc=1, w_sh=w_sh, w_sp=w_sp)
    d = xcorr_desc(n, h, wd, c, oc, kh, kw, stride, padding, dilation, groups, act, act_param, per_sample,
                   x_sn=h * x_sh, x_sh=x_sh, x_sp=x_sp, y_sn=ho * y_sh, y_sh=y_sh, y_sp=y_sp, **wst)
    dx, dw = DeviceBuffer.from_numpy(xw), DeviceBuffer.from_numpy(ww)
    dy = DeviceBuffer.from_numpy(yw, out=True)
    db = DeviceBuffer.from_numpy(_f32(b)) if b is not None else None
    px, pw, py = dx.ptr + x.itemsize * x_off, dw.ptr + x.itemsize * w_off, dy.ptr + x.itemsize * y_off
    LAST_KERNEL_NAME["si_hip_xcorr"] = H.si_hip_xcorr_kernel_name(C.byref(d), C.c_void_p(px), C.c_void_p(pw), C.c_void_p(py), 1 if half else 0).decode()
    name = "si_hip_xcorr_f16" if half else "si_hip_xcorr_f32"
    _chk(getattr(H, name)(C.byref(d), px, pw, db.ptr if db else None, py, None), name)
    y = dy.to_numpy(yw.shape, x.dtype)
    if full:
        return y
    return np.ascontiguousarray(y[:, :, out_w_off:out_w_off + wo, out_c_off:out_c_off + oc])


def xcorr_kernel_name(n, h, w, c, oc, kh, kw, stride=1, padding=0, dilation=1, groups=1, half=False, per_sample=False) -> str:
    """the instantiation for dense tensors at aligned addresses; "none": a refused descriptor"""
    d = xcorr_desc(n, h, w, c, oc, kh, kw, stride, padding, dilation, groups, per_sample=per_sample)
    return _native.hip().si_hip_xcorr_kernel_name(C.byref(d), C.c_void_p(1 << 24), C.c_void_p(1 << 28), C.c_void_p(1 << 30), 1 if half else 0).decode()


REDUCE_OPS = {"sum": 0, "mean": 1, "amax": 2, "amin": 3}


def reduce_out_shape(x_shape, axes):
    """the NHWC output shape of a reduction over the mask `axes` (1 n, 2 h, 4 w, 8 c): every reduced axis has extent 1"""
    return tuple(1 if (int(axes) >> a) & 1 else int(v) for a, v in enumerate(x_shape))


def reduce_desc(x_shape, op, axes, in_ld=None, out_ld=None):
    """SiReduceDesc (include/si_reduce.h) of an NHWC input; op: a name of REDUCE_OPS or the code; axes: the bit mask"""
    n, h, w, c = x_shape
    oc = 1 if int(axes) & 8 else c
    return _native.SiReduceDesc(n, h, w, c, in_ld or c, out_ld or oc, int(axes), REDUCE_OPS[op] if isinstance(op, str) else int(op))


def reduce(x, op, axes, in_ld=None, in_c_off=0, in_fill=0.0, out_ld=None, out_c_off=0, out_fill=0.0, full=False):
    """si_hip_reduce_f32 / _f16 (by the array's dtype) on an NHWC array: torch.sum / mean / amax / amin (`op`) over the NHWC axes of the
    bit mask `axes` (1 n, 2 h, 4 w, 8 c), keepdim=True.  The view hooks are the common ones."""
    x = _float_storage(x)
    assert x.ndim == 4, "NHWC (a rank-2 [N, F] array is [N, 1, 1, F])"
    d = reduce_desc(x.shape, op, axes, in_ld, out_ld)
    oshape = reduce_out_shape(x.shape, axes if 1 <= int(axes) <= 15 else 0)
    return _run_desc_op("reduce", d, x, oshape[:-1], oshape[3], in_ld, in_c_off, in_fill, out_ld, out_c_off, out_fill, full)


def reduce_kernel_name(x_shape, op, axes, half=False, in_ld=None, out_ld=None) -> str:
    """the instantiation for 16-byte aligned buffers of these shapes ("none": a descriptor the launch refuses)"""
    d = reduce_desc(x_shape, op, axes, in_ld, out_ld)
    return _desc_kernel_name("reduce", d, half)


LPNORM_P = {1: 0, 2: 1, float("inf"): 2}


def lpnorm_desc(x_shape, p, axes, normalize=False, eps=0.0, in_ld=None, out_ld=None):
    """SiLpNormDesc (include/si_lpnorm.h) of an NHWC input; p: 1, 2 or inf (or, as an int outside those, the raw code); axes: the bit mask"""
    n, h, w, c = x_shape
    oc = c if normalize or not int(axes) & 8 else 1
    code = LPNORM_P[float(p)] if float(p) in LPNORM_P else int(p)
    return _native.SiLpNormDesc(n, h, w, c, in_ld or c, out_ld or oc, int(axes), code, int(normalize), float(eps))


def lpnorm(x, p, axes, normalize=False, eps=0.0, in_ld=None, in_c_off=0, in_fill=0.0, out_ld=None, out_c_off=0, out_fill=0.0, full=False):
    """si_hip_lpnorm_f32 / _f16 (by the array's dtype) on an NHWC array: torch.norm(p) over the NHWC axes of the bit mask `axes` (1 n, 2 h,
    4 w, 8 c), keepdim=True, or -- normalize -- F.normalize(p, eps) along the one axis of the mask.  The view hooks are the common ones."""
    x = _float_storage(x)
    assert x.ndim == 4, "NHWC (a rank-2 [N, F] array is [N, 1, 1, F])"
    d = lpnorm_desc(x.shape, p, axes, normalize, eps, in_ld, out_ld)
    oshape = tuple(x.shape) if normalize else reduce_out_shape(x.shape, axes if 1 <= int(axes) <= 15 else 0)
    return _run_desc_op("lpnorm", d, x, oshape[:-1], oshape[3], in_ld, in_c_off, in_fill, out_ld, out_c_off, out_fill, full)


def lpnorm_kernel_name(x_shape, p, axes, normalize=False, half=False, in_ld=None, out_ld=None) -> str:
    """the instantiation for 16-byte aligned buffers of these shapes ("none": a descriptor the launch refuses)"""
    return _desc_kernel_name("lpnorm", lpnorm_desc(x_shape, p, axes, normalize, 0.0, in_ld, out_ld), half)


PARAM_ACT_OPS = {"clamp": 0, "softplus": 1, "mish": 2}


def param_act_desc(x_shape, op, p0=0.0, p1=0.0, in_ld=None, out_ld=None):
    """SiParamActDesc (include/si_act.h) of an array whose last axis is the channels; op: a name of PARAM_ACT_OPS or the code"""
    c = int(x_shape[-1])
    pixels = int(np.prod(x_shape[:-1], dtype=np.int64)) if len(x_shape) > 1 else 1
    return _native.SiParamActDesc(PARAM_ACT_OPS[op] if isinstance(op, str) else int(op), float(p0), float(p1), pixels, c, in_ld or c, out_ld or c)


def param_act(x, op, p0=0.0, p1=0.0, half=False, in_ld=None, in_c_off=0, in_fill=0.0, out_ld=None, out_c_off=0, out_fill=0.0, full=False):
    """si_hip_param_act_f32 / _f16 (half=True, or a float16 array) on an array whose last axis is the channels: clamp (p0 lo, p1 hi),
    softplus (p0 beta, p1 threshold) or mish.  The view hooks are the common ones."""
    x = np.asarray(x)
    x = np.ascontiguousarray(x, dtype=np.float16) if (half or x.dtype == np.float16) else _f32(x)
    d = param_act_desc(x.shape, op, p0, p1, in_ld, out_ld)
    return _run_desc_op("param_act", d, x, x.shape[:-1], x.shape[-1], in_ld, in_c_off, in_fill, out_ld, out_c_off, out_fill, full)


def param_act_kernel_name(x_shape, op, p0=0.0, p1=0.0, half=False, in_ld=None, out_ld=None) -> str:
    """the instantiation for 16-byte aligned buffers of these shapes ("none": a descriptor the launch refuses)"""
    d = param_act_desc(x_shape, op, p0, p1, in_ld, out_ld)
    return _desc_kernel_name("param_act", d, half)


def pixel_shuffle_desc(x_shape, r, inverse=False, in_ld=None, out_ld=None):
    """SiPixelShuffleDesc (include/si_superres.h) of an NHWC input; the output shape is the rule's (floor division: a height, width or
    channel count the factor does not divide gives a descriptor the entry refuses)"""
    n, ih, iw, ic = (int(v) for v in x_shape)
    r = int(r)
    q = max(r, 1)
    oh, ow, oc = (ih // q, iw // q, ic * r * r) if inverse else (ih * r, iw * r, ic // (q * q))
    return _native.SiPixelShuffleDesc(n, ih, iw, ic, in_ld or ic, oh, ow, oc, out_ld or oc, r, 1 if inverse else 0)


def pixel_shuffle(x_nhwc, r, inverse=False, in_ld=None, in_c_off=0, in_fill=0.0, out_ld=None, out_c_off=0, out_fill=0.0, full=False):
    """si_hip_pixel_shuffle_f32 / _f16 (by the array's dtype) on an NHWC array: torch.nn.functional.pixel_shuffle(x, r) of the NCHW
    tensor, or pixel_unshuffle with inverse=True.  The array's bits travel as they are.  The view hooks are the common ones."""
    x = _float_storage(x_nhwc)
    d = pixel_shuffle_desc(x.shape, r, inverse, in_ld, out_ld)
    if d.oh < 1 or d.ow < 1 or d.oc < 1:
        raise HipError("si_hip_pixel_shuffle: factor %d leaves no output for a %r input" % (r, tuple(x.shape)))
    return _run_desc_op("pixel_shuffle", d, x, (d.n, d.oh, d.ow), d.oc, in_ld, in_c_off, in_fill, out_ld, out_c_off, out_fill, full)


def pixel_shuffle_kernel_name(x_shape, r, inverse=False, half=False, in_ld=None, out_ld=None) -> str:
    """the form for 16-byte aligned buffers of these shapes ("none": a descriptor the launch refuses)"""
    d = pixel_shuffle_desc(x_shape, r, inverse, in_ld, out_ld)
    return _desc_kernel_name("pixel_shuffle", d, half)


def prelu(x, slope, in_ld=None, in_c_off=0, in_fill=0.0, out_ld=None, out_c_off=0, out_fill=0.0, full=False):
    """si_hip_prelu_f32 / _f16 (by the array's dtype) on an array whose last axis is the channels (NHWC, or [N, F]):
    torch.nn.functional.prelu with `slope` of 1 or C fp32 elements.  The view hooks are the common ones."""
    H = _native.hip()
    x = _float_storage(x)
    half = x.dtype == np.float16
    c = x.shape[-1]
    slope = _f32(slope).reshape(-1)
    ds = DeviceBuffer.from_numpy(slope)
    (dx, px), (dy, py) = _view_in(x, in_ld, in_c_off, in_fill), _view_out(x.shape[:-1], c, out_ld, out_c_off, out_fill, x.dtype)
    LAST_KERNEL_NAME["si_hip_prelu"] = H.si_hip_prelu_kernel_name(C.c_void_p(px), x.size // c, c, in_ld or c, slope.size, C.c_void_p(py), out_ld or c,
                                                                  1 if half else 0).decode()
    fn, name = (H.si_hip_prelu_f16, "si_hip_prelu_f16") if half else (H.si_hip_prelu_f32, "si_hip_prelu_f32")
    _chk(fn(px, x.size // c, c, in_ld or c, ds.ptr, slope.size, py, out_ld or c, None), name)
    return _ret(dy.to_numpy(x.shape[:-1] + (out_ld or c,), x.dtype), c, out_c_off, full)


def prelu_kernel_name(x_shape, slope_count=1, half=False, in_ld=None, out_ld=None) -> str:
    """the instantiation for 16-byte aligned buffers of this shape ("none": arguments the launch refuses)"""
    c = int(x_shape[-1])
    pixels = int(np.prod(x_shape[:-1], dtype=np.int64))
    return _native.hip().si_hip_prelu_kernel_name(C.c_void_p(256), pixels, c, in_ld or c, int(slope_count), C.c_void_p(256), out_ld or c,
                                                  1 if half else 0).decode()


_ALL = slice(None)   # (the builtin: this module's own slice() is defined below)


def slice_desc(x_shape, index, in_ld=None, out_ld=None):
    """SiSliceDesc (include/si_slice.h) of an NHWC input (or [N, F]: taken as [N, 1, 1, F]) and `index`, one Python slice per axis in the
    array's own order with steps >= 1 -- the descriptor of x[index]"""
    shape = tuple(int(v) for v in x_shape)
    index = tuple(index) + (_ALL,) * (len(shape) - len(index))
    if len(shape) == 2:
        shape, index = (shape[0], 1, 1, shape[1]), (index[0], _ALL, _ALL, index[1])
    rng = [range(*s.indices(n)) for s, n in zip(index, shape)]
    assert all(r.step >= 1 for r in rng), "steps are at least 1"
    d = _native.SiSliceDesc()
    d.n, d.ih, d.iw, d.ic = shape
    d.on, d.oh, d.ow, d.oc = (len(r) for r in rng)
    for a, r in enumerate(rng):
        d.start[a], d.step[a] = r.start, r.step
    d.in_ld, d.out_ld = in_ld or d.ic, out_ld or d.oc
    return d


def slice(x, index, in_ld=None, in_c_off=0, in_fill=0.0, out_ld=None, out_c_off=0, out_fill=0.0, full=False):
    """si_hip_slice_f32 / _f16 (by the array's dtype): x[index] of an NHWC (or [N, F]) array, index as in slice_desc.  The array's bits
    travel as they are.  The view hooks are the common ones."""
    x = _float_storage(x)
    d = slice_desc(x.shape, index, in_ld, out_ld)
    if min(d.on, d.oh, d.ow, d.oc) < 1:
        raise HipError("si_hip_slice: %r of a %r input is empty" % (index, tuple(x.shape)))
    oshape = (d.on, d.oh, d.ow) if x.ndim == 4 else (d.on,)
    return _run_desc_op("slice", d, x, oshape, d.oc, in_ld, in_c_off, in_fill, out_ld, out_c_off, out_fill, full)


def slice_kernel_name(x_shape, index, half=False, in_ld=None, out_ld=None) -> str:
    """the form for 16-byte aligned buffers of these shapes ("none": a descriptor the launch refuses)"""
    d = slice_desc(x_shape, index, in_ld, out_ld)
    return _desc_kernel_name("slice", d, half)


def _split_args(widths, offsets, out_lds, ptrs):
    k = len(widths)
    if offsets is None:
        offsets = [int(sum(widths[:i])) for i in range(k)]
    ia = lambda v: (C.c_int * k)(*[int(t) for t in v])
    return k, ia(offsets), ia(widths), (C.c_void_p * k)(*ptrs), ia(out_lds)


def split_channels(x, widths, offsets=None, in_ld=None, in_c_off=0, in_fill=0.0, out_lds=None, out_c_offs=None, out_fill=0.0, full=False):
    """si_hip_split_channels_f32 / _f16 (by the array's dtype): one call that copies channels [offsets[i], offsets[i] + widths[i]) of an array
    whose last axis is the channels into destination i (offsets default to the widths laid end to end: torch.split).  Returns the list of
    destinations.  out_lds / out_c_offs: one pixel stride / channel offset per destination; the other view hooks are the common ones."""
    H = _native.hip()
    x = _float_storage(x)
    half = x.dtype == np.float16
    c, k = x.shape[-1], len(widths)
    out_lds = [int(v) if v else int(w) for v, w in zip(out_lds or [None] * k, widths)]
    out_c_offs = list(out_c_offs or [0] * k)
    dx, px = _view_in(x, in_ld, in_c_off, in_fill)
    outs = [_view_out(x.shape[:-1], int(w), ld, co, out_fill, x.dtype) for w, ld, co in zip(widths, out_lds, out_c_offs)]
    args = (px, x.size // c, c, in_ld or c) + _split_args(widths, offsets, out_lds, [py for _, py in outs])
    LAST_KERNEL_NAME["si_hip_split_channels"] = H.si_hip_split_channels_kernel_name(*(args + (1 if half else 0,))).decode()
    fn, name = (H.si_hip_split_channels_f16, "si_hip_split_channels_f16") if half else (H.si_hip_split_channels_f32, "si_hip_split_channels_f32")
    _chk(fn(*(args + (None,))), name)
    return [_ret(dy.to_numpy(x.shape[:-1] + (ld,), x.dtype), int(w), co, full) for (dy, _), w, ld, co in zip(outs, widths, out_lds, out_c_offs)]


def split_channels_kernel_name(x_shape, widths, offsets=None, half=False, in_ld=None, out_lds=None) -> str:
    """the form for 16-byte aligned buffers of these shapes ("none": arguments the launch refuses)"""
    c = int(x_shape[-1])
    pixels = int(np.prod(x_shape[:-1], dtype=np.int64))
    k = len(widths)
    out_lds = [int(v) if v else int(w) for v, w in zip(out_lds or [None] * k, widths)]
    args = (C.c_void_p(256), pixels, c, in_ld or c) + _split_args(widths, offsets, out_lds, [256] * k)
    return _native.hip().si_hip_split_channels_kernel_name(*(args + (1 if half else 0,))).decode()


PERMUTE_FORMS = {"auto": 0, "rows": 1, "tile": 2, "elem": 3}
LAYOUT_OPS = {"permute": 0, "reshape": 1, "view": 1, "transpose": 2, "squeeze": 3, "unsqueeze": 4, "contiguous": 5}


def permute_desc(dims, in_stride, out_ld=None, form=0):
    """SiPermuteDesc (include/si_permute.h): the output loop nest `dims`, outermost first, with the input element stride of every loop
    dimension; out_ld defaults to the dense pitch dims[-1]"""
    d = _native.SiPermuteDesc()
    d.rank = len(dims)
    for k in range(min(len(dims), 4)):
        d.dims[k], d.in_stride[k] = int(dims[k]), int(in_stride[k])
    d.out_ld = int(out_ld) if out_ld else (int(dims[-1]) if len(dims) else 0)
    d.form = PERMUTE_FORMS.get(form, form)
    return d


def permute_ref(src, desc, out_ld=None, out_fill=0):
    """numpy statement of the descriptor on the flat source array: [runs, out_ld] with out_fill where nothing is written"""
    dims = [desc.dims[k] for k in range(desc.rank)]
    st = [desc.in_stride[k] for k in range(desc.rank)]
    idx = np.zeros(dims, np.int64)
    for k, (n, s) in enumerate(zip(dims, st)):
        idx += (np.arange(n, dtype=np.int64) * s).reshape([n if j == k else 1 for j in range(len(dims))])
    runs = int(np.prod(dims[:-1], dtype=np.int64))
    out = _full((runs, out_ld or desc.out_ld), src.dtype, out_fill)
    out[:, :dims[-1]] = np.asarray(src).reshape(-1)[idx.reshape(runs, dims[-1])]
    return out


def permute(src, desc, half=False, form=None, src_off=0, out_off=0, out_fill=0.0):
    """si_hip_permute_f32 / _f16 (half, or a float16 array): the flat array `src` is uploaded as it is and the kernel is handed the pointer
    src_off elements into it; the destination is out_off + runs * out_ld elements pre-filled with out_fill (a value or a ByteFill), the kernel
    writing from out_off on.  Returns the [runs, out_ld] rows behind out_off: what lies between two runs must still hold out_fill.  form: a
    key of PERMUTE_FORMS to force, None: the descriptor's.  The array's bits travel as they are; under guard_bands() both buffers are banded."""
    H = _native.hip()
    src = np.ascontiguousarray(np.asarray(src).reshape(-1))
    if half and src.dtype != np.float16:
        src = src.astype(np.float16)
    src = _float_storage(src)
    half = src.dtype == np.float16
    if form is not None:
        desc.form = PERMUTE_FORMS.get(form, form)
    runs = int(np.prod([desc.dims[k] for k in range(desc.rank - 1)], dtype=np.int64))
    dx = DeviceBuffer.from_numpy(src)
    dy = DeviceBuffer.from_numpy(_full((int(out_off) + runs * desc.out_ld,), src.dtype, out_fill), out=True)
    px, py = dx.ptr + src.itemsize * int(src_off), dy.ptr + src.itemsize * int(out_off)
    LAST_KERNEL_NAME["si_hip_permute"] = H.si_hip_permute_kernel_name(C.byref(desc), C.c_void_p(px), C.c_void_p(py), 1 if half else 0).decode()
    fn, name = (H.si_hip_permute_f16, "si_hip_permute_f16") if half else (H.si_hip_permute_f32, "si_hip_permute_f32")
    _chk(fn(C.byref(desc), px, py, None), name)
    return dy.to_numpy((int(out_off) + runs * desc.out_ld,), src.dtype)[int(out_off):].reshape(runs, desc.out_ld)


def permute_kernel_name(desc, half=False, src_align=256, dst_align=256) -> str:
    """the form for buffers at these addresses (256: 16-byte aligned; "none": a descriptor the launch refuses)"""
    return _native.hip().si_hip_permute_kernel_name(C.byref(desc), C.c_void_p(src_align), C.c_void_p(dst_align), 1 if half else 0).decode()


def layout_plan(in_shape, ops, out_shape=None, in_ld=0):
    """si_layout_plan (include/si_layout.h): the layout algebra over file-order shapes.  ops: [(name, args)], name a key of LAYOUT_OPS.  Returns
    (status, view, dims, in_stride): status 0 / 3 kErrorShape / 5 kUnsupport; for a nest of more than 4 dimensions (5) dims still holds it."""
    L = _native.host()
    ia = lambda v: (C.c_int * max(len(v), 1))(*[int(t) for t in v])
    kinds = [LAYOUT_OPS[k] for k, _ in ops]
    args = [int(a) for _, aa in ops for a in (aa if isinstance(aa, (tuple, list)) else [aa])]
    nargs = [len(aa) if isinstance(aa, (tuple, list)) else 1 for _, aa in ops]
    nest = _native.SiLayoutNest()
    out_shape = list(out_shape) if out_shape is not None else []
    rc = L.si_layout_plan(len(in_shape), ia(in_shape), int(in_ld), len(ops), ia(kinds), ia(nargs), ia(args), len(out_shape), ia(out_shape),
                          C.byref(nest))
    r = min(nest.rank, len(nest.dims))
    return rc, bool(nest.view), [nest.dims[k] for k in range(r)], [nest.in_stride[k] for k in range(r)]


def flatten_nhwc(x, in_ld=None, in_c_off=0, in_fill=0.0, out_fill=None):
    """out_fill: as cat()"""
    H = _native.hip()
    x = _f32(x)
    n, h, w, c = x.shape
    (dx, px), dy = _view_in(x, in_ld, in_c_off, in_fill), (DeviceBuffer(x.nbytes) if out_fill is None else
                                                           DeviceBuffer.from_numpy(_full((x.size,), np.float32, out_fill), out=True))
    _chk(H.si_hip_nhwc_to_nchw_f32(px, n, h, w, c, in_ld or c, dy.ptr, None), "si_hip_nhwc_to_nchw_f32")
    return dy.to_numpy((n, c * h * w))


def yolo_detect(feats, weights, biases, grids, anchor_grids, strides, na=3, fused=False, in_pad=0, in_c_off=0, in_fill=0.0):
    """Detect head exactly as the YoloDetect layer runs it: per level 1x1 conv kernel + decode kernel, or (fused)
    si_hip_conv2d_yolo_f32 -- the conv with the decode + concat in its epilogue."""
    H = _native.hip()
    if fused:
        return _yolo_detect_fused(feats, weights, biases, grids, anchor_grids, strides, na, in_pad=in_pad, in_c_off=in_c_off, in_fill=in_fill)
    feats = [_f32(f) for f in feats]
    n = feats[0].shape[0]
    ne = weights[0].shape[0] // na
    rows_total = sum(f.shape[1] * f.shape[2] * na for f in feats)
    dout = DeviceBuffer(n * rows_total * ne * 4)
    off = 0
    for f, w, b, g, a, s in zip(feats, weights, biases, grids, anchor_grids, strides):
        _, h, wd, cin = f.shape
        conv = conv2d(f, w, b)  # [n,h,w,na*ne]
        g2 = _f32(np.transpose(_f32(g)[0], (1, 2, 0, 3)))   # [na,h,w,2] -> [h,w,na,2] (yolo_detect.cpp:75-79)
        a2 = _f32(np.transpose(_f32(a)[0], (1, 2, 0, 3)))
        dc, dg, da = DeviceBuffer.from_numpy(conv), DeviceBuffer.from_numpy(g2), DeviceBuffer.from_numpy(a2)
        _chk(H.si_hip_yolo_decode_f32(dc.ptr, n, h, wd, na, ne, dg.ptr, da.ptr, float(s), dout.ptr, rows_total, off, None),
             "si_hip_yolo_decode_f32")
        sync()
        off += h * wd * na
    return dout.to_numpy((n, rows_total, ne))


def yolo_detect_split3(feats, weights, biases, grids, anchor_grids, strides, na=3, return_flags=False, in_pad=0, in_c_off=0, in_fill=0.0):
    """si_hip_conv2d_split3_yolo_f32 per level: the Detect head on the f32_split arithmetic (fp32 features, three fp16 MFMA products per
    fp32 product), decode + concat in the epilogue.  return_flags: also the per-level range-guard words."""
    return _yolo_detect_fused(feats, weights, biases, grids, anchor_grids, strides, na, split3=True, return_flags=return_flags, in_pad=in_pad,
                              in_c_off=in_c_off, in_fill=in_fill)


def _yolo_detect_fused(feats, weights, biases, grids, anchor_grids, strides, na, split3=False, return_flags=False, in_pad=0, in_c_off=0, in_fill=0.0):
    """in_pad / in_c_off: every level's features as channels [in_c_off, in_c_off + C) of rows of C + in_pad elements (the gap holds in_fill)"""
    from ._native import SiYoloLevel
    H = _native.hip()
    feats = [_f32(f) for f in feats]
    n = feats[0].shape[0]
    ne = weights[0].shape[0] // na
    rows_total = sum(f.shape[1] * f.shape[2] * na for f in feats)
    dout = DeviceBuffer(n * rows_total * ne * 4)
    dout.fill(0)
    off = 0
    flags = []
    for f, w, b, g, a, s in zip(feats, weights, biases, grids, anchor_grids, strides):
        _, h, wd, cin = f.shape
        w = _f32(w)
        d = SiConv2dDesc(n, h, wd, cin, cin + in_pad, h, wd, na * ne, na * ne, 1, 1, 1, 1, 1, 1, 0, 0, 1, 1, 0, 0, na * ne, 0, 0.0)
        if split3:
            packed = np.zeros(H.si_hip_conv2d_split3_weight_elems(C.byref(d)), np.float16)
            _chk(H.si_hip_conv2d_split3_pack_weight_host(C.byref(d), w.ctypes.data_as(C.c_void_p), packed.ctypes.data_as(C.c_void_p)), "pack")
        else:
            packed = np.zeros(H.si_hip_conv2d_weight_elems(C.byref(d)), np.float32)
            _chk(H.si_hip_conv2d_pack_weight_host(C.byref(d), w.ctypes.data_as(C.c_void_p), packed.ctypes.data_as(C.c_void_p)), "pack")
        g2 = _f32(np.transpose(_f32(g)[0], (1, 2, 0, 3)))
        a2 = _f32(np.transpose(_f32(a)[0], (1, 2, 0, 3)))
        bufs = [None] + [DeviceBuffer.from_numpy(v) for v in (packed, _f32(b), g2, a2)]
        bufs[0], pf = _view_in(f, cin + in_pad, in_c_off, in_fill)
        lv = SiYoloLevel(na, ne, rows_total, off, float(s))
        fn = H.si_hip_conv2d_split3_yolo_f32 if split3 else H.si_hip_conv2d_yolo_f32
        flag = _range_flag(d, return_flags and split3)
        _chk(fn(C.byref(d), pf, bufs[1].ptr, bufs[2].ptr, C.byref(lv), bufs[3].ptr, bufs[4].ptr, dout.ptr, None),
             "si_hip_conv2d_split3_yolo_f32" if split3 else "si_hip_conv2d_yolo_f32")
        sync()
        if flag is not None:
            flags.append(int(flag.to_numpy((1,), np.uint32)[0]))
        off += h * wd * na
    out = dout.to_numpy((n, rows_total, ne))
    return (out, flags) if return_flags else out


def letterbox_geometry(height_origin, width_origin, height_new, width_new):
    """(height_resize, width_resize, scale, padding_t, padding_l) of PreProcess (test_yolo.cpp:194-241)."""
    hr, wr, pt, pl = C.c_int(), C.c_int(), C.c_int(), C.c_int()
    sc = C.c_float()
    _native.hip().si_letterbox_geometry(height_origin, width_origin, height_new, width_new, C.byref(hr), C.byref(wr),
                                        C.byref(sc), C.byref(pt), C.byref(pl))
    return hr.value, wr.value, sc.value, pt.value, pl.value


def letterbox(resized_bgr, height_new, width_new, padding_t, padding_l):
    """u8 BGR [hr][wr][3] -> float RGB [height_new][width_new][3], padded with 114, / 255 (test_yolo.cpp:220-259)."""
    H = _native.hip()
    src = np.ascontiguousarray(resized_bgr, dtype=np.uint8)
    hr, wr = int(src.shape[0]), int(src.shape[1])
    dsrc = DeviceBuffer.from_numpy(src)
    dout = DeviceBuffer(height_new * width_new * 3 * 4)
    _chk(H.si_hip_letterbox_u8_f32(dsrc.ptr, hr, wr, dout.ptr, height_new, width_new, padding_t, padding_l, None),
         "si_hip_letterbox_u8_f32")
    return dout.to_numpy((height_new, width_new, 3))


def _strided_images(src, stride, fill):
    """u8 images [n][...] -> host bytes [n][stride], image b at b * stride, the gap behind each image filled with the byte `fill`"""
    n = int(src.shape[0])
    per = int(src.size // n) if n else 0
    if stride is None:
        return src, per          # dense: uploaded as it is
    stride = int(stride)
    assert stride >= per, "an image stride shorter than the image"
    host = np.full((n, stride), fill, np.uint8)
    host[:, :per] = src.reshape(n, per)
    return host, stride


def letterbox_batch(resized_bgr, height_new, width_new, padding_t, padding_l, src_stride=None, src_fill=0):
    """si_hip_letterbox_batch_u8_f32: u8 BGR [n][hr][wr][3] -> float RGB [n][height_new][width_new][3] in one launch.  src_stride: image
    stride of the source in bytes (default: dense), the gaps filled with the byte src_fill."""
    H = _native.hip()
    src = np.ascontiguousarray(resized_bgr, dtype=np.uint8)
    n, hr, wr = int(src.shape[0]), int(src.shape[1]), int(src.shape[2])
    host, stride = _strided_images(src, src_stride, src_fill)
    dsrc = DeviceBuffer.from_numpy(host)
    dout = DeviceBuffer(max(n * height_new * width_new * 3 * 4, 16))
    _chk(H.si_hip_letterbox_batch_u8_f32(dsrc.ptr, n, stride, hr, wr, dout.ptr, height_new, width_new, padding_t, padding_l, None),
         "si_hip_letterbox_batch_u8_f32")
    return dout.to_numpy((n, height_new, width_new, 3))


def resize_bilinear_u8c3(images, dst_h, dst_w, src_stride=None, src_fill=0, dst_stride=None, dst_fill=0, full=False):
    """si_hip_resize_bilinear_u8c3: u8 [n][h][w][3] -> u8 [n][dst_h][dst_w][3] (the cv::resize of PreProcess, test_yolo.cpp:213-216).
    src_stride / dst_stride: image strides in bytes (default: dense), the gaps filled with the bytes src_fill / dst_fill before the launch;
    full: return the destination as it lies in memory, bytes [n][dst_stride], gaps included."""
    H = _native.hip()
    src = np.ascontiguousarray(images, dtype=np.uint8)
    n, h, w = int(src.shape[0]), int(src.shape[1]), int(src.shape[2])
    host, sstride = _strided_images(src, src_stride, src_fill)
    per = dst_h * dst_w * 3
    dstride = per if dst_stride is None else int(dst_stride)
    assert dstride >= per, "an image stride shorter than the image"
    dsrc = DeviceBuffer.from_numpy(host)
    if dst_stride is None:
        dout = DeviceBuffer(max(n * dstride, 16))          # dense: every byte is written, nothing to pre-fill
    else:
        dout = DeviceBuffer.from_numpy(np.full(max(n * dstride, 16), dst_fill, np.uint8), out=True)
    _chk(H.si_hip_resize_bilinear_u8c3(dsrc.ptr, n, sstride, h, w, dout.ptr, dstride, dst_h, dst_w, None), "si_hip_resize_bilinear_u8c3")
    raw = dout.to_numpy((n, dstride), np.uint8)
    return raw if full else np.ascontiguousarray(raw[:, :per]).reshape(n, dst_h, dst_w, 3)


def resize_letterbox_batch(frames_bgr, height_new, width_new, src_stride=None, src_fill=0):
    """si_hip_resize_letterbox_batch_u8_f32: camera frames u8 BGR [n][h][w][3] -> float RGB [n][height_new][width_new][3]
    (aspect-preserving bilinear resize + pad(114) + / 255: PreProcess whole, test_yolo.cpp:194-259) in one launch.  src_stride: image
    stride of the frames in bytes (default: dense), the gaps filled with the byte src_fill."""
    H = _native.hip()
    src = np.ascontiguousarray(frames_bgr, dtype=np.uint8)
    n, h, w = int(src.shape[0]), int(src.shape[1]), int(src.shape[2])
    host, stride = _strided_images(src, src_stride, src_fill)
    dsrc = DeviceBuffer.from_numpy(host)
    dout = DeviceBuffer(max(n * height_new * width_new * 3 * 4, 16))
    _chk(H.si_hip_resize_letterbox_batch_u8_f32(dsrc.ptr, n, stride, h, w, dout.ptr, height_new, width_new, None),
         "si_hip_resize_letterbox_batch_u8_f32")
    return dout.to_numpy((n, height_new, width_new, 3))


def yolo_postprocess(pred, prob_threshold=0.25, nms_threshold=0.45, agnostic=False, adjust=None, max_det=None,
                     pred_dev=None, workspace=None, dets_dev=None):
    """Device post-processing of test_yolo.cpp:337-428.  pred [n][rows][ne] -> list (one per image) of float arrays
    [k][6] = {x, y, w, h, confidence, label} in picked order.  adjust: None or [n][5]
    {padding_l, padding_t, scale, image cols, image rows}.  workspace: a caller's DeviceBuffer to use as the scratch (at least
    si_hip_yolo_postprocess_workspace_bytes; whatever it holds must not matter); dets_dev: a caller's DeviceBuffer for the
    [n][max_det][6] output, so that the caller can see what the entry left untouched in it.  Both default to fresh buffers."""
    H = _native.hip()
    pred = _f32(pred)
    n, rows, ne = (int(v) for v in pred.shape)
    if max_det is None:
        max_det = max(rows, 1)
    dpred = pred_dev if pred_dev is not None else DeviceBuffer.from_numpy(pred)
    dadj = DeviceBuffer.from_numpy(_f32(adjust).reshape(n, 5)) if adjust is not None else None
    wsb = H.si_hip_yolo_postprocess_workspace_bytes(n, rows, ne)
    dws = workspace if workspace is not None else DeviceBuffer(wsb)
    assert dws.nbytes >= wsb, "workspace of %d bytes, the call needs %d" % (dws.nbytes, wsb)
    ddets = dets_dev if dets_dev is not None else DeviceBuffer(max(n * max_det * 6 * 4, 16))
    assert ddets.nbytes >= n * max_det * 6 * 4, "dets buffer of %d bytes, the call needs %d" % (ddets.nbytes, n * max_det * 6 * 4)
    dcnt = DeviceBuffer(max(n * 4, 16))
    _chk(H.si_hip_yolo_postprocess_f32(dpred.ptr, n, rows, ne, float(prob_threshold), float(nms_threshold),
                                       int(bool(agnostic)), dadj.ptr if dadj else None, ddets.ptr, dcnt.ptr, max_det,
                                       dws.ptr, dws.nbytes, None), "si_hip_yolo_postprocess_f32")
    if n == 0:
        return [], np.zeros((0,), np.int32)
    cnt = dcnt.to_numpy((n,), np.int32)
    dets = ddets.to_numpy((n, max_det, 6)) if max_det > 0 else np.zeros((n, 0, 6), np.float32)
    return [dets[b, :min(int(cnt[b]), max_det)].copy() for b in range(n)], cnt


# ---- include/si_detect.h: post-processing for anchor-free heads, payloads and instance masks -------------------------------------------------
DETECT_LAYOUTS = {"rows": 0, "channels": 1}
DETECT_BOX_FORMATS = {"cxcywh": 0, "xyxy": 1}


def detect_desc(n, rows, classes, objectness=False, extra=0, layout="rows", box_format="cxcywh", prob_threshold=0.25, nms_threshold=0.45,
                agnostic=False, max_det=None, ld=None, image_ld=None):
    """SiDetectPostDesc; ld / image_ld default to the dense strides of the layout, max_det to rows"""
    ne = 4 + int(bool(objectness)) + int(classes) + int(extra)
    lay = DETECT_LAYOUTS[layout] if isinstance(layout, str) else int(layout)
    fmt = DETECT_BOX_FORMATS[box_format] if isinstance(box_format, str) else int(box_format)
    if ld is None:
        ld = rows if lay == 1 else ne
    if image_ld is None:
        image_ld = ne * ld if lay == 1 else rows * ld
    return _native.SiDetectPostDesc(int(n), int(rows), int(classes), int(bool(objectness)), int(extra), lay, int(ld), int(image_ld), fmt,
                                    float(prob_threshold), float(nms_threshold), int(bool(agnostic)), int(rows if max_det is None else max_det))


def detect_filter_kernel_name(d, pred_ptr=256) -> str:
    return _native.hip().si_hip_detect_filter_kernel_name(C.byref(d), C.c_void_p(pred_ptr)).decode()


def detect_workspace_bytes(d) -> int:
    return int(_native.hip().si_hip_detect_postprocess_workspace_bytes(C.byref(d)))


def detect_storage(pred, layout="rows", ld=None, image_ld=None, offset=0, fill=np.nan):
    """the flat fp32 storage of a logical pred ([n][rows][ne] for "rows", [n][ne][rows] for "channels") with row / channel stride ld, image stride
    image_ld and `offset` leading elements; every gap holds `fill`"""
    pred = _f32(pred)
    n, outer, inner = pred.shape
    ld = inner if ld is None else int(ld)
    image_ld = outer * ld if image_ld is None else int(image_ld)
    assert ld >= inner and image_ld >= (outer - 1) * ld + inner
    flat = _full((offset + (n - 1) * image_ld + (outer - 1) * ld + inner,), np.float32, fill)
    for b in range(n):
        for o in range(outer):
            at = offset + b * image_ld + o * ld
            flat[at:at + inner] = pred[b, o]
    return flat


class DetectResult:
    """what detect_postprocess returns: per-image lists cut to min(counts[b], max_det) (dets [k][6], src_rows [k], net_boxes [k][4], extras
    [k][extra]; None for an output that was not asked for), counts [n], `full`: the whole output arrays as read back, `dev`: their device
    buffers (for detect_masks), `max_det`, `extra`"""

    def __init__(self, n, max_det, extra, counts, full, dev):
        self.n, self.max_det, self.extra, self.counts, self.full, self.dev = n, max_det, extra, counts, full, dev
        k = [min(int(c), max_det) for c in counts]
        for name in ("dets", "src_rows", "net_boxes", "extras"):
            a = full.get(name)
            setattr(self, name, None if a is None else [a[b, :k[b]].copy() for b in range(n)])


def detect_postprocess(pred, classes, objectness=False, extra=0, layout="rows", box_format="cxcywh", prob_threshold=0.25, nms_threshold=0.45,
                       agnostic=False, adjust=None, max_det=None, pred_dev=None, ld=None, image_ld=None, workspace=None, shape=None, pred_off=0,
                       in_fill=np.nan, want=("src_rows", "net_boxes", "extras"), host=None, out_fill=0.0, stream=None):
    """si_hip_detect_postprocess_f32 (include/si_detect.h).  pred: the logical array, [n][rows][ne] for layout "rows" and [n][ne][rows] for
    "channels"; ld / image_ld / pred_off lay it out with gaps (filled with in_fill) and a base pointer pred_off elements into the buffer.
    pred_dev: a DeviceBuffer (or a view on an Engine.extract pointer with outputs_to_host=0) that already holds the storage, with
    shape = (n, rows); pred is then not read.  want: which optional outputs to ask for; host: which outputs to copy to the host (None: all that
    exist; counts always) -- the others stay on the device in the result's `dev`, where detect_masks finds them.  out_fill: what the output buffers hold before the
    call (a value or a ByteFill), so that a caller sees what was left untouched.  Returns a DetectResult."""
    H = _native.hip()
    lay = DETECT_LAYOUTS[layout]
    if pred_dev is None:
        pred = _f32(pred)
        n, rows = (pred.shape[0], pred.shape[2]) if lay == 1 else (pred.shape[0], pred.shape[1])
        dbuf = DeviceBuffer.from_numpy(detect_storage(pred, layout, ld, image_ld, pred_off, in_fill))
        pred_ptr = dbuf.ptr + 4 * pred_off
    else:
        n, rows = (int(v) for v in shape)
        pred_ptr = pred_dev.ptr + 4 * pred_off
    d = detect_desc(n, rows, classes, objectness, extra, layout, box_format, prob_threshold, nms_threshold, agnostic, max_det, ld, image_ld)
    max_det = d.max_det
    dadj = DeviceBuffer.from_numpy(_f32(adjust).reshape(n, 5)) if adjust is not None else None
    wsb = detect_workspace_bytes(d)
    dws = workspace if workspace is not None else DeviceBuffer(max(wsb, 16))
    assert wsb == 0 or dws.nbytes >= wsb, "workspace of %d bytes, the call needs %d" % (dws.nbytes, wsb)
    shapes = {"dets": ((n, max_det, 6), np.float32), "counts": ((n,), np.int32), "src_rows": ((n, max_det), np.int32),
              "net_boxes": ((n, max_det, 4), np.float32), "extras": ((n, max_det, int(extra)), np.float32)}
    dev = {}
    for name, (shp, dt) in shapes.items():
        if name in ("dets", "counts") or name in want:
            dev[name] = DeviceBuffer.from_numpy(_full((max(int(np.prod(shp)), 4),), dt, out_fill), out=True)
    out = _native.SiDetectPostOut(*[dev[k].ptr if k in dev else None for k in ("dets", "counts", "src_rows", "net_boxes", "extras")])
    _chk(H.si_hip_detect_postprocess_f32(C.byref(d), pred_ptr, dadj.ptr if dadj else None, C.byref(out), dws.ptr, dws.nbytes, stream),
         "si_hip_detect_postprocess_f32")
    full = {k: b.to_numpy(shapes[k][0], shapes[k][1], stream) for k, b in dev.items() if host is None or k in host or k == "counts"}
    return DetectResult(n, max_det, int(extra), full["counts"].copy(), full, dev)


def detect_mask_desc(n, mh, mw, nm, max_det, extra, coef_off=0, ratio_w=0.25, ratio_h=0.25, proto_ld=None):
    return _native.SiDetectMaskDesc(int(n), int(mh), int(mw), int(nm), int(nm if proto_ld is None else proto_ld), int(max_det), int(extra),
                                    int(coef_off), float(np.float32(ratio_w)), float(np.float32(ratio_h)))


def detect_masks_kernel_name(d, protos_ptr=256) -> str:
    return _native.hip().si_hip_detect_masks_kernel_name(C.byref(d), C.c_void_p(protos_ptr)).decode()


def detect_masks(protos, extras, net_boxes, counts, ratio_w=0.25, ratio_h=0.25, coef_off=0, nm=None, proto_ld=None, protos_dev=None, shape=None,
                 protos_off=0, in_fill=np.nan, out_fill=0, full=False, stream=None):
    """si_hip_detect_masks_f32.  protos: [n][mh][mw][nm] (NHWC), laid out with pixel stride proto_ld (gaps: in_fill) and protos_off leading
    elements -- or protos_dev, a DeviceBuffer that holds them (an Engine.extract pointer with outputs_to_host=0), with shape = (n, mh, mw, nm).
    extras [n][max_det][extra], net_boxes [n][max_det][4] and counts [n] are numpy arrays -- or pass a DetectResult as `extras` (net_boxes and
    counts are then ignored): its device buffers are read where detect_postprocess left them.  Returns, per image, the planes
    [min(counts[b], max_det)][mh][mw] uint8, the only bytes copied back -- or with full=True the whole [n][max_det][mh][mw] buffer as read
    back (pre-filled with the byte out_fill)."""
    H = _native.hip()
    if isinstance(extras, DetectResult):
        res = extras
        max_det, extra = res.max_det, res.extra
        dext, dbox, dcnt, cnt = res.dev["extras"], res.dev["net_boxes"], res.dev["counts"], res.counts
    else:
        extras, net_boxes, cnt = _f32(extras), _f32(net_boxes), np.ascontiguousarray(counts, np.int32)
        max_det, extra = int(extras.shape[1]), int(extras.shape[2])
        dext = DeviceBuffer.from_numpy(extras if extras.size else np.zeros(4, np.float32))
        dbox = DeviceBuffer.from_numpy(net_boxes if net_boxes.size else np.zeros(4, np.float32))
        dcnt = DeviceBuffer.from_numpy(cnt)
    if protos_dev is None:
        protos = _f32(protos)
        n, mh, mw, pnm = (int(v) for v in protos.shape)
        ldp = pnm if proto_ld is None else int(proto_ld)
        store = _full((protos_off + n * mh * mw * ldp,), np.float32, in_fill)
        store[protos_off:].reshape(n * mh * mw, ldp)[:, :pnm] = protos.reshape(-1, pnm)
        dpro = DeviceBuffer.from_numpy(store)
    else:
        n, mh, mw, pnm = (int(v) for v in shape)
        ldp = pnm if proto_ld is None else int(proto_ld)
        dpro = protos_dev
    nm = pnm if nm is None else int(nm)
    d = detect_mask_desc(n, mh, mw, nm, max_det, extra, coef_off, ratio_w, ratio_h, ldp)
    dmask = DeviceBuffer.from_numpy(np.full(max(n * max_det * mh * mw, 16), out_fill, np.uint8), out=True)
    _chk(H.si_hip_detect_masks_f32(C.byref(d), dpro.ptr + 4 * protos_off, dext.ptr, dbox.ptr, dcnt.ptr, dmask.ptr, stream), "si_hip_detect_masks_f32")
    if full:
        return dmask.to_numpy((n, max_det, mh, mw), np.uint8, stream)
    # the planes of the kept detections alone leave the device
    kept = [min(int(cnt[b]), max_det) for b in range(n)]
    return [DeviceBuffer.view(dmask.ptr + b * max_det * mh * mw, max(kept[b] * mh * mw, 16)).to_numpy((kept[b], mh, mw), np.uint8, stream) for b in range(n)]


# ---------------------------------------------------------------------------
# fp16 storage path (include/si_hip.h "fp16 storage path").  Activations travel as numpy float16 (IEEE binary16, the
# device's _Float16); results come back as float16 unless noted.
# ---------------------------------------------------------------------------
def _f16(a) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=np.float16)


def conv2d_f16(x, w_oihw, bias=None, stride=(1, 1), padding=(0, 0), dilation=(1, 1), groups=1, act1="none",
               residual=None, act2="none", act_param=0.0, in_ld=None, out_ld=None, out_c_off=0, out_f32=False, in_fill=0.0, in_c_off=0,
               res_ld=None, res_c_off=0, res_fill=0.0, out_fill=0.0, full=False):
    """si_hip_conv2d_f16, si_hip_conv2d_stem_f16 when the shape is a stem (fp32 image in, fp16 out), or si_hip_conv2d_depthwise_f16.
    in_fill: what lies between the pixels' channels of a strided (in_ld > ic) input."""
    H = _native.hip()
    w_oihw = _f32(w_oihw)
    n, ih, iw, ic = x.shape
    oc, _, kh, kw = w_oihw.shape
    oh, ow = conv_out_hw(ih, iw, (kh, kw), stride, padding, dilation)
    in_ld = in_ld or ic
    out_ld = out_ld or oc
    d = SiConv2dDesc(n, ih, iw, ic, in_ld, oh, ow, oc, out_ld, kh, kw, stride[0], stride[1], dilation[0], dilation[1],
                     padding[0], padding[1], groups, 1 if bias is not None else 0, ACT[act1],
                     1 if residual is not None else 0, res_ld or oc, ACT[act2], float(act_param))
    kind = H.si_hip_conv2d_f16_supported(C.byref(d))
    if kind == 0:
        raise HipError("no fp16 conv kernel for this shape")
    db = DeviceBuffer.from_numpy(_f32(bias)) if bias is not None else None
    odt = np.float32 if out_f32 else np.float16
    dy, py = _view_out((n, oh, ow), oc, out_ld, out_c_off, out_fill, odt)
    if kind == 2:
        packed = np.zeros(H.si_hip_conv2d_stem_f16_weight_elems(C.byref(d)), np.float16)
        _chk(H.si_hip_conv2d_stem_f16_pack_weight_host(C.byref(d), w_oihw.ctypes.data_as(C.c_void_p),
                                                       packed.ctypes.data_as(C.c_void_p)), "pack stem f16")
        (dx, px), dw = _view_in(_f32(x), in_ld, in_c_off, in_fill), DeviceBuffer.from_numpy(packed)
        _chk(H.si_hip_conv2d_stem_f16(C.byref(d), px, dw.ptr, db.ptr if db else None, py, None), "si_hip_conv2d_stem_f16")
        return _ret(dy.to_numpy((n, oh, ow, out_ld), np.float16), oc, out_c_off, full)
    if kind == 3:   # depthwise: fp16 activations, the FP32 depthwise weight image
        packed = np.zeros(H.si_hip_conv2d_weight_elems(C.byref(d)), np.float32)
        _chk(H.si_hip_conv2d_pack_weight_host(C.byref(d), w_oihw.ctypes.data_as(C.c_void_p), packed.ctypes.data_as(C.c_void_p)), "pack depthwise")
        if out_f32:
            raise HipError("the fp16 depthwise kernel writes fp16")
        (dx, px), dw = _view_in(_f16(x), in_ld, in_c_off, in_fill), DeviceBuffer.from_numpy(packed)
        dr, pr = _view_in(_f16(residual), res_ld, res_c_off, res_fill) if residual is not None else (None, None)
        _chk(H.si_hip_conv2d_depthwise_f16(C.byref(d), px, dw.ptr, db.ptr if db else None, pr, py, None), "si_hip_conv2d_depthwise_f16")
        return _ret(dy.to_numpy((n, oh, ow, out_ld), np.float16), oc, out_c_off, full)
    packed = np.zeros(H.si_hip_conv2d_f16_weight_elems(C.byref(d)), np.float16)
    _chk(H.si_hip_conv2d_f16_pack_weight_host(C.byref(d), w_oihw.ctypes.data_as(C.c_void_p), packed.ctypes.data_as(C.c_void_p)), "pack f16")
    (dx, px), dw = _view_in(_f16(x), in_ld, in_c_off, in_fill), DeviceBuffer.from_numpy(packed)
    dr, pr = _view_in(_f16(residual), res_ld, res_c_off, res_fill) if residual is not None else (None, None)
    LAST_KERNEL_NAME["si_hip_conv2d_f16"] = H.si_hip_conv2d_f16_kernel_name(C.byref(d), 0).decode()
    LAST_KERNEL_NAME["f16_tile_variant"] = int(H.si_hip_conv2d_f16_tile_variant(C.byref(d)))
    _chk(H.si_hip_conv2d_f16(C.byref(d), px, dw.ptr, db.ptr if db else None, pr, py, 1 if out_f32 else 0, None), "si_hip_conv2d_f16")
    return _ret(dy.to_numpy((n, oh, ow, out_ld), odt), oc, out_c_off, full)


def conv2d_split_f16(x, w_a, b_a, w_b, b_b, act1="none", in_ld=None, in_c_off=0, in_fill=0.0, out_ld=None, out_c_off=0, out2_ld=None, out2_c_off=0,
                     out_fill=0.0, full=False):
    H = _native.hip()
    x = _f16(x)
    n, h, w, ic = x.shape
    oa, ob = w_a.shape[0], w_b.shape[0]
    wcat = _f32(np.concatenate([w_a, w_b], 0))
    bcat = _f32(np.concatenate([b_a, b_b], 0))
    out_ld, out2_ld = out_ld or oa, out2_ld or ob
    d = SiConv2dDesc(n, h, w, ic, in_ld or ic, h, w, oa + ob, out_ld, 1, 1, 1, 1, 1, 1, 0, 0, 1, 1, ACT[act1], 0, oa, 0, 0.0)
    packed = np.zeros(H.si_hip_conv2d_f16_weight_elems(C.byref(d)), np.float16)
    _chk(H.si_hip_conv2d_f16_pack_weight_host(C.byref(d), wcat.ctypes.data_as(C.c_void_p), packed.ctypes.data_as(C.c_void_p)), "pack f16")
    (dx, px), dw, db = _view_in(x, in_ld, in_c_off, in_fill), DeviceBuffer.from_numpy(packed), DeviceBuffer.from_numpy(bcat)
    (dy, py), (dy2, py2) = (_view_out((n, h, w), oa, out_ld, out_c_off, out_fill, np.float16),
                            _view_out((n, h, w), ob, out2_ld, out2_c_off, out_fill, np.float16))
    _chk(H.si_hip_conv2d_split_f16(C.byref(d), px, dw.ptr, db.ptr, py, oa, py2, out2_ld, None), "si_hip_conv2d_split_f16")
    return (_ret(dy.to_numpy((n, h, w, out_ld), np.float16), oa, out_c_off, full),
            _ret(dy2.to_numpy((n, h, w, out2_ld), np.float16), ob, out2_c_off, full))


def maxpool2d_f16(x, k, s, p, d=(1, 1), in_ld=None, in_c_off=0, in_fill=0.0, out_ld=None, out_c_off=0, out_fill=0.0, full=False):
    H = _native.hip()
    x = _f16(x)
    n, ih, iw, c = x.shape
    oh, ow = conv_out_hw(ih, iw, k, s, p, d)
    desc = SiPool2dDesc(n, ih, iw, c, in_ld or c, oh, ow, out_ld or c, k[0], k[1], s[0], s[1], d[0], d[1], p[0], p[1])
    (dx, px), (dy, py) = _view_in(x, in_ld, in_c_off, in_fill), _view_out((n, oh, ow), c, out_ld, out_c_off, out_fill, np.float16)
    _chk(H.si_hip_maxpool2d_f16(C.byref(desc), px, py, None), "si_hip_maxpool2d_f16")
    return _ret(dy.to_numpy((n, oh, ow, out_ld or c), np.float16), c, out_c_off, full)


def adaptive_avgpool2d_f16(x, out_hw, in_ld=None, in_c_off=0, in_fill=0.0, out_ld=None, out_c_off=0, out_fill=0.0, full=False):
    H = _native.hip()
    x = _f16(x)
    n, ih, iw, c = x.shape
    (dx, px), (dy, py) = _view_in(x, in_ld, in_c_off, in_fill), _view_out((n, out_hw[0], out_hw[1]), c, out_ld, out_c_off, out_fill, np.float16)
    _chk(H.si_hip_adaptive_avgpool2d_f16(px, n, ih, iw, c, in_ld or c, py, out_hw[0], out_hw[1], out_ld or c, None),
         "si_hip_adaptive_avgpool2d_f16")
    return _ret(dy.to_numpy((n, out_hw[0], out_hw[1], out_ld or c), np.float16), c, out_c_off, full)


def activation_f16(kind, x, param=0.0, in_ld=None, in_c_off=0, in_fill=0.0, out_ld=None, out_c_off=0, out_fill=0.0, full=False):
    H = _native.hip()
    x = _f16(x)
    c = x.shape[-1]
    pixels = x.size // c
    (dx, px), (dy, py) = _view_in(x, in_ld, in_c_off, in_fill), _view_out(x.shape[:-1], c, out_ld, out_c_off, out_fill, np.float16)
    _chk(H.si_hip_activation_f16(ACT[kind], float(param), px, pixels, c, in_ld or c, py, out_ld or c, None), "si_hip_activation_f16")
    return _ret(dy.to_numpy(x.shape[:-1] + (out_ld or c,), np.float16), c, out_c_off, full)


def binary_same_f16(op, a, b, in_ld=None, in_c_off=0, in_fill=0.0, out_ld=None, out_c_off=0, out_fill=0.0, full=False, b_ld=None, b_c_off=0):
    """si_hip_binary_same_f16; in_ld / in_c_off are a's view, b_ld / b_c_off b's (both gaps hold in_fill)"""
    H = _native.hip()
    a, b = _f16(a), _f16(b)
    c = a.shape[-1]
    pixels = a.size // c
    (da, pa), (db, pb) = _view_in(a, in_ld, in_c_off, in_fill), _view_in(b, b_ld, b_c_off, in_fill)
    dy, py = _view_out(a.shape[:-1], c, out_ld, out_c_off, out_fill, np.float16)
    _chk(H.si_hip_binary_same_f16({"add": 0, "mul": 2}[op], pa, in_ld or c, pb, b_ld or c, py, out_ld or c, pixels, c, None),
         "si_hip_binary_same_f16")
    return _ret(dy.to_numpy(a.shape[:-1] + (out_ld or c,), np.float16), c, out_c_off, full)


def binary_bcast_f16(op, a, s, in_ld=None, in_c_off=0, in_fill=0.0, out_ld=None, out_c_off=0, out_fill=0.0, full=False):
    """si_hip_binary_bcast_f16: a [n][h][w][c] (op) s [n][c] broadcast over h, w (the squeeze-excite scale)."""
    H = _native.hip()
    a, s = _f16(a), _f16(s)
    n, c = a.shape[0], a.shape[-1]
    ppi = a.size // (n * c)
    (da, pa), ds, (dy, py) = _view_in(a, in_ld, in_c_off, in_fill), DeviceBuffer.from_numpy(s), _view_out(a.shape[:-1], c, out_ld, out_c_off, out_fill, np.float16)
    _chk(H.si_hip_binary_bcast_f16({"add": 0, "mul": 2}[op], pa, in_ld or c, ds.ptr, c, py, out_ld or c, n, ppi, c, None), "si_hip_binary_bcast_f16")
    return _ret(dy.to_numpy(a.shape[:-1] + (out_ld or c,), np.float16), c, out_c_off, full)


def convert_roundtrip_f16(x, in_ld=None, in_c_off=0, in_fill=0.0, out_ld=None, out_c_off=0, out_fill=0.0, full=False):
    """fp32 -> fp16 -> fp32 on the device (si_hip_convert_f32_f16 / si_hip_convert_f16_f32); the views are those of the fp32 input and of BOTH
    destinations (the fp16 intermediate is read back as the slice of its rows)."""
    H = _native.hip()
    x = _f32(x)
    c = x.shape[-1]
    pixels = x.size // c
    old = out_ld or c
    dx, px = _view_in(x, in_ld, in_c_off, in_fill)
    (dh, ph), (dy, py) = _view_out(x.shape[:-1], c, old, out_c_off, out_fill, np.float16), _view_out(x.shape[:-1], c, old, out_c_off, out_fill)
    _chk(H.si_hip_convert_f32_f16(px, pixels, c, in_ld or c, ph, old, None), "si_hip_convert_f32_f16")
    half = _ret(dh.to_numpy(x.shape[:-1] + (old,), np.float16), c, out_c_off, full)
    _chk(H.si_hip_convert_f16_f32(ph, pixels, c, old, py, old, None), "si_hip_convert_f16_f32")
    return half, _ret(dy.to_numpy(x.shape[:-1] + (old,)), c, out_c_off, full)


def conv_stem_s2c32_f16(x, w0, b0, w1, b1, out_ld=None, out_c_off=0, out_fill=0.0, full=False):
    """si_hip_conv2d_stem_s2c32_f16: YOLOv5's first two convs (6x6 s2 p2 3 -> 32 SiLU, 3x3 s2 p1 32 -> oc SiLU) in one launch.
    x fp32 [n][h][w][3]; returns fp16 [n][oh][ow][oc]."""
    H = _native.hip()
    x, w0, w1 = _f32(x), _f32(w0), _f32(w1)
    n, ih, iw, _ = x.shape
    sh_, sw_ = conv_out_hw(ih, iw, (6, 6), (2, 2), (2, 2), (1, 1))
    oh, ow = conv_out_hw(sh_, sw_, (3, 3), (2, 2), (1, 1), (1, 1))
    oc = w1.shape[0]
    d0 = SiConv2dDesc(n, ih, iw, 3, 3, sh_, sw_, 32, 32, 6, 6, 2, 2, 1, 1, 2, 2, 1, 1 if b0 is not None else 0, ACT["silu"], 0, 32, 0, 0.0)
    d1 = SiConv2dDesc(n, sh_, sw_, 32, 32, oh, ow, oc, out_ld or oc, 3, 3, 2, 2, 1, 1, 1, 1, 1, 1 if b1 is not None else 0, ACT["silu"], 0, oc, 0, 0.0)
    if not H.si_hip_conv2d_stem_s2c32_f16_supported(C.byref(d0), C.byref(d1)):
        raise HipError("si_hip_conv2d_stem_s2c32_f16: unsupported shape")
    p0 = np.zeros(H.si_hip_conv2d_stem_f16_weight_elems(C.byref(d0)), np.float16)
    _chk(H.si_hip_conv2d_stem_f16_pack_weight_host(C.byref(d0), w0.ctypes.data_as(C.c_void_p), p0.ctypes.data_as(C.c_void_p)), "pack stem f16")
    p1 = np.zeros(H.si_hip_conv2d_f16_weight_elems(C.byref(d1)), np.float16)
    _chk(H.si_hip_conv2d_f16_pack_weight_host(C.byref(d1), w1.ctypes.data_as(C.c_void_p), p1.ctypes.data_as(C.c_void_p)), "pack f16")
    dx, dp0, dp1 = DeviceBuffer.from_numpy(x), DeviceBuffer.from_numpy(p0), DeviceBuffer.from_numpy(p1)
    db0 = DeviceBuffer.from_numpy(_f32(b0)) if b0 is not None else None
    db1 = DeviceBuffer.from_numpy(_f32(b1)) if b1 is not None else None
    dy, py = _view_out((n, oh, ow), oc, out_ld, out_c_off, out_fill, np.float16)
    _chk(H.si_hip_conv2d_stem_s2c32_f16(C.byref(d0), C.byref(d1), dx.ptr, dp0.ptr, db0.ptr if db0 else None, dp1.ptr,
                                        db1.ptr if db1 else None, py, None), "si_hip_conv2d_stem_s2c32_f16")
    sync()
    return _ret(dy.to_numpy((n, oh, ow, out_ld or oc), np.float16), oc, out_c_off, full)


def conv_stem_s2c32_pw_f16(x, w0, b0, w1, b1, w2, b2, split_oc=32, out2_ld=None, out2_c_off=0, out_ld=None, out_c_off=0, out_fill=0.0, full=False):
    """si_hip_conv2d_stem_s2c32_pw_f16: YOLOv5's first two convs AND the 1x1 conv behind them (64 -> 64, SiLU: the first C3's cv1 | cv2 over the
    concatenated filters w2 [64][64][1][1]) in one launch.  x fp32 [n][h][w][3].  split_oc = 32: returns (fp16 [n][oh][ow][32], fp16
    [n][oh][ow][32]) -- the second one written at channel offset out2_c_off of a buffer with pixel stride out2_ld; split_oc = 0: one fp16
    [n][oh][ow][64]."""
    H = _native.hip()
    x, w0, w1, w2 = _f32(x), _f32(w0), _f32(w1), _f32(w2)
    n, ih, iw, _ = x.shape
    sh_, sw_ = conv_out_hw(ih, iw, (6, 6), (2, 2), (2, 2), (1, 1))
    oh, ow = conv_out_hw(sh_, sw_, (3, 3), (2, 2), (1, 1), (1, 1))
    oc = w1.shape[0]
    d0 = SiConv2dDesc(n, ih, iw, 3, 3, sh_, sw_, 32, 32, 6, 6, 2, 2, 1, 1, 2, 2, 1, 1 if b0 is not None else 0, ACT["silu"], 0, 32, 0, 0.0)
    d1 = SiConv2dDesc(n, sh_, sw_, 32, 32, oh, ow, oc, oc, 3, 3, 2, 2, 1, 1, 1, 1, 1, 1 if b1 is not None else 0, ACT["silu"], 0, oc, 0, 0.0)
    c_a = 32 if split_oc else 64
    ld_a = out_ld or c_a
    d2 = SiConv2dDesc(n, oh, ow, oc, oc, oh, ow, 64, ld_a, 1, 1, 1, 1, 1, 1, 0, 0, 1, 1 if b2 is not None else 0, ACT["silu"], 0, 64, 0, 0.0)
    if not H.si_hip_conv2d_stem_s2c32_pw_f16_supported(C.byref(d0), C.byref(d1), C.byref(d2), split_oc):
        raise HipError("si_hip_conv2d_stem_s2c32_pw_f16: unsupported shape")
    p0 = np.zeros(H.si_hip_conv2d_stem_f16_weight_elems(C.byref(d0)), np.float16)
    _chk(H.si_hip_conv2d_stem_f16_pack_weight_host(C.byref(d0), w0.ctypes.data_as(C.c_void_p), p0.ctypes.data_as(C.c_void_p)), "pack stem f16")
    p1 = np.zeros(H.si_hip_conv2d_f16_weight_elems(C.byref(d1)), np.float16)
    _chk(H.si_hip_conv2d_f16_pack_weight_host(C.byref(d1), w1.ctypes.data_as(C.c_void_p), p1.ctypes.data_as(C.c_void_p)), "pack f16")
    p2 = np.zeros(H.si_hip_conv2d_f16_weight_elems(C.byref(d2)), np.float16)
    _chk(H.si_hip_conv2d_f16_pack_weight_host(C.byref(d2), w2.ctypes.data_as(C.c_void_p), p2.ctypes.data_as(C.c_void_p)), "pack f16")
    bufs = [DeviceBuffer.from_numpy(v) for v in (x, p0, p1, p2)]
    db = [DeviceBuffer.from_numpy(_f32(b)) if b is not None else None for b in (b0, b1, b2)]
    out2_ld = out2_ld or 32
    (dy, py), (dy2, py2) = (_view_out((n, oh, ow), c_a, ld_a, out_c_off, out_fill, np.float16),
                            _view_out((n, oh, ow), 32, out2_ld, out2_c_off, out_fill, np.float16))
    _chk(H.si_hip_conv2d_stem_s2c32_pw_f16(C.byref(d0), C.byref(d1), C.byref(d2), bufs[0].ptr, bufs[1].ptr, db[0].ptr if db[0] else None, bufs[2].ptr,
                                           db[1].ptr if db[1] else None, bufs[3].ptr, db[2].ptr if db[2] else None, py, split_oc,
                                           py2 if split_oc else None, out2_ld, None), "si_hip_conv2d_stem_s2c32_pw_f16")
    sync()
    ya = _ret(dy.to_numpy((n, oh, ow, ld_a), np.float16), c_a, out_c_off, full)
    if not split_oc:
        return ya
    return ya, _ret(dy2.to_numpy((n, oh, ow, out2_ld), np.float16), 32, out2_c_off, full)


def conv_pw_slab_f16(x, w0, b0, w1, b1, residual=None, out_ld=None, out_c_off=0, in_ld=None, in_c_off=0, in_fill=0.0, res_ld=None, res_c_off=0,
                     res_fill=0.0, out_fill=0.0, full=False):
    """si_hip_conv2d_pw_slab_f16: the C3 bottleneck's two convs (1x1 c -> c SiLU, 3x3 s1 p1 c -> oc SiLU, optional shortcut) in one
    launch.  x NHWC fp16; returns NHWC fp16."""
    H = _native.hip()
    x, w0, w1 = _f16(x), _f32(w0), _f32(w1)
    n, ih, iw, c = x.shape
    oc = w1.shape[0]
    in_ld = in_ld or c
    out_ld = out_ld or oc
    d0 = SiConv2dDesc(n, ih, iw, c, in_ld, ih, iw, c, c, 1, 1, 1, 1, 1, 1, 0, 0, 1, 1 if b0 is not None else 0, ACT["silu"], 0, c, 0, 0.0)
    d1 = SiConv2dDesc(n, ih, iw, c, c, ih, iw, oc, out_ld, 3, 3, 1, 1, 1, 1, 1, 1, 1, 1 if b1 is not None else 0, ACT["silu"],
                      1 if residual is not None else 0, res_ld or oc, 0, 0.0)
    if not H.si_hip_conv2d_pw_slab_f16_supported(C.byref(d0), C.byref(d1)):
        raise HipError("si_hip_conv2d_pw_slab_f16: unsupported shape")
    p0 = np.zeros(H.si_hip_conv2d_f16_weight_elems(C.byref(d0)), np.float16)
    _chk(H.si_hip_conv2d_f16_pack_weight_host(C.byref(d0), w0.ctypes.data_as(C.c_void_p), p0.ctypes.data_as(C.c_void_p)), "pack 1x1")
    p1 = np.zeros(H.si_hip_conv2d_f16_weight_elems(C.byref(d1)), np.float16)
    _chk(H.si_hip_conv2d_f16_pack_weight_host(C.byref(d1), w1.ctypes.data_as(C.c_void_p), p1.ctypes.data_as(C.c_void_p)), "pack 3x3")
    (dx, px), dp0, dp1 = _view_in(x, in_ld, in_c_off, in_fill), DeviceBuffer.from_numpy(p0), DeviceBuffer.from_numpy(p1)
    db0 = DeviceBuffer.from_numpy(_f32(b0)) if b0 is not None else None
    db1 = DeviceBuffer.from_numpy(_f32(b1)) if b1 is not None else None
    dr, pr = _view_in(_f16(residual), res_ld, res_c_off, res_fill) if residual is not None else (None, None)
    dy, py = _view_out((n, ih, iw), oc, out_ld, out_c_off, out_fill, np.float16)
    _chk(H.si_hip_conv2d_pw_slab_f16(C.byref(d0), C.byref(d1), px, dp0.ptr, db0.ptr if db0 else None, dp1.ptr, db1.ptr if db1 else None,
                                     pr, py, None), "si_hip_conv2d_pw_slab_f16")
    sync()
    return _ret(dy.to_numpy((n, ih, iw, out_ld), np.float16), oc, out_c_off, full)


def conv_pw_cv3_f16(x, w0, b0, w1, b1, z, w3, b3, residual=None, z_ld=None, z_c_off=0, out_ld=None, out_c_off=0, z_fill=0.0, in_ld=None, in_c_off=0,
                    in_fill=0.0, res_ld=None, res_c_off=0, res_fill=0.0, out_fill=0.0, full=False):
    """si_hip_conv2d_pw_cv3_f16: a C3's last bottleneck pair (1x1 c -> c SiLU, 3x3 c -> c SiLU, optional shortcut) AND the C3's closing 1x1
    conv over cat([pair output, z]) in one launch (c = 64, z 64 channels, w3 [128][128][1][1]).  x, z, residual NHWC fp16; returns NHWC fp16
    [n][h][w][128].  z_ld / z_c_off: z read as a channel slice of a wider buffer."""
    H = _native.hip()
    x, z, w0, w1, w3 = _f16(x), _f16(z), _f32(w0), _f32(w1), _f32(w3)
    n, ih, iw, c = x.shape
    oc3 = w3.shape[0]
    z_ld = z_ld or z.shape[-1]
    out_ld = out_ld or oc3
    d0 = SiConv2dDesc(n, ih, iw, c, in_ld or c, ih, iw, c, c, 1, 1, 1, 1, 1, 1, 0, 0, 1, 1 if b0 is not None else 0, ACT["silu"], 0, c, 0, 0.0)
    d1 = SiConv2dDesc(n, ih, iw, c, c, ih, iw, c, c, 3, 3, 1, 1, 1, 1, 1, 1, 1, 1 if b1 is not None else 0, ACT["silu"],
                      1 if residual is not None else 0, res_ld or c, 0, 0.0)
    d2 = SiConv2dDesc(n, ih, iw, 2 * c, 2 * c, ih, iw, oc3, out_ld, 1, 1, 1, 1, 1, 1, 0, 0, 1, 1 if b3 is not None else 0, ACT["silu"], 0, oc3, 0, 0.0)
    if not H.si_hip_conv2d_pw_cv3_f16_supported(C.byref(d0), C.byref(d1), C.byref(d2)):
        raise HipError("si_hip_conv2d_pw_cv3_f16: unsupported shape")
    packs = []
    for d, w in ((d0, w0), (d1, w1), (d2, w3)):
        p = np.zeros(H.si_hip_conv2d_f16_weight_elems(C.byref(d)), np.float16)
        _chk(H.si_hip_conv2d_f16_pack_weight_host(C.byref(d), w.ctypes.data_as(C.c_void_p), p.ctypes.data_as(C.c_void_p)), "pack f16")
        packs.append(DeviceBuffer.from_numpy(p))
    (dx, px), (dz, pz) = _view_in(x, in_ld, in_c_off, in_fill), _view_in(z, z_ld, z_c_off, z_fill)
    db = [DeviceBuffer.from_numpy(_f32(b)) if b is not None else None for b in (b0, b1, b3)]
    dr, pr = _view_in(_f16(residual), res_ld, res_c_off, res_fill) if residual is not None else (None, None)
    dy, py = _view_out((n, ih, iw), oc3, out_ld, out_c_off, out_fill, np.float16)
    _chk(H.si_hip_conv2d_pw_cv3_f16(C.byref(d0), C.byref(d1), C.byref(d2), px, packs[0].ptr, db[0].ptr if db[0] else None, packs[1].ptr,
                                    db[1].ptr if db[1] else None, pr, pz, z_ld, packs[2].ptr,
                                    db[2].ptr if db[2] else None, py, None), "si_hip_conv2d_pw_cv3_f16")
    sync()
    return _ret(dy.to_numpy((n, ih, iw, out_ld), np.float16), oc3, out_c_off, full)


def yolo_f16_tile(x_shape, na, ne, rows_total=None) -> int:
    """si_hip_conv2d_yolo_f16_tile: the form si_hip_conv2d_yolo_f16 launches for a Detect level over an NHWC feature map of x_shape
    (1: the Detect tile, 0: the generic tiles)"""
    n, h, w, cin = x_shape
    d = SiConv2dDesc(n, h, w, cin, cin, h, w, na * ne, na * ne, 1, 1, 1, 1, 1, 1, 0, 0, 1, 1, 0, 0, na * ne, 0, 0.0)
    lv = _native.SiYoloLevel(na, ne, rows_total or h * w * na, 0, 8.0)
    LAST_ENTRIES.append("si_hip_conv2d_yolo_f16_tile")
    return int(_native.hip().si_hip_conv2d_yolo_f16_tile(C.byref(d), C.byref(lv)))


def yolo_detect_f16(feats, weights, biases, grids, anchor_grids, strides, na=3, in_pad=0, in_c_off=0, in_fill=0.0):
    """si_hip_conv2d_yolo_f16 per level: fp16 features, fp32 [n][rows_total][ne] detections."""
    H = _native.hip()
    feats = [_f16(f) for f in feats]
    n = feats[0].shape[0]
    ne = weights[0].shape[0] // na
    rows_total = sum(f.shape[1] * f.shape[2] * na for f in feats)
    dout = DeviceBuffer(n * rows_total * ne * 4)
    off = 0
    for f, w, b, g, a, s in zip(feats, weights, biases, grids, anchor_grids, strides):
        _, h, wd, cin = f.shape
        w = _f32(w)
        d = SiConv2dDesc(n, h, wd, cin, cin + in_pad, h, wd, na * ne, na * ne, 1, 1, 1, 1, 1, 1, 0, 0, 1, 1, 0, 0, na * ne, 0, 0.0)
        packed = np.zeros(H.si_hip_conv2d_f16_weight_elems(C.byref(d)), np.float16)
        _chk(H.si_hip_conv2d_f16_pack_weight_host(C.byref(d), w.ctypes.data_as(C.c_void_p), packed.ctypes.data_as(C.c_void_p)), "pack")
        g2 = _f32(np.transpose(_f32(g)[0], (1, 2, 0, 3)))
        a2 = _f32(np.transpose(_f32(a)[0], (1, 2, 0, 3)))
        bufs = [None] + [DeviceBuffer.from_numpy(v) for v in (packed, _f32(b), g2, a2)]
        bufs[0], pf = _view_in(f, cin + in_pad, in_c_off, in_fill)
        lv = _native.SiYoloLevel(na, ne, rows_total, off, float(s))
        _chk(H.si_hip_conv2d_yolo_f16(C.byref(d), pf, bufs[1].ptr, bufs[2].ptr, C.byref(lv), bufs[3].ptr, bufs[4].ptr,
                                      dout.ptr, None), "si_hip_conv2d_yolo_f16")
        sync()
        off += h * wd * na
    return dout.to_numpy((n, rows_total, ne))
