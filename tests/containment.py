"""Containment checks: what a kernel may touch given a view (ptr, ld, c), and the matrix of cases that drives every compute entry of the
C-ABI (include/si_hip.h) through them.  Pure numpy: the checkers and the completeness rule run without a GPU (tests/test_containment_cpu.py);
the cases run in tests/test_gpu_containment.py under simpleinfer_amd.hipops.guard_bands.

A case is data: an id, the C entries it drives, an optional kernel-form plan, and a function run(hops, F) that calls one hipops wrapper with
every gap (in_fill / res_fill / z_fill / out_fill) set to the fill F and returns the destinations as Out(name, full buffer, c_off, c).  Nothing
here has a tolerance: every assertion is equality of bits."""
import os
import re

import numpy as np

PATTERNS = (0xFF, 0x7B)   # NaN as fp32 / fp16, 255 as u8  |  1.3e36 as fp32, 61280 as fp16, 123 as u8 (wins every max: v_max drops a NaN operand)
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "si_hip.h")


# ---- checkers ------------------------------------------------------------------------------------------------------------------------------
def _bits(a):
    """a's bytes as uint8 [..., itemsize per element] (NaN fills must compare equal: never compare floats)"""
    a = np.ascontiguousarray(a)
    return a.view(np.uint8).reshape(a.shape + (a.dtype.itemsize,))


def _where(idx, shape):
    """'pixel (..), channel c' of a flat element index into an array whose last axis is the channel"""
    pos = np.unravel_index(int(idx), shape)
    return "pixel %s, channel %d" % ("(" + ", ".join(str(int(p)) for p in pos[:-1]) + ")", int(pos[-1]))


def assert_outside_fill(full, c_off, c, byte, what=""):
    """every byte of the row buffer `full` [..., ld] outside channels [c_off, c_off + c) equals `byte`"""
    full = np.asarray(full)
    ld = full.shape[-1]
    assert 0 <= c_off and c_off + c <= ld, (c_off, c, ld)
    bad = (_bits(full) != np.uint8(byte)).any(axis=-1)
    bad[..., c_off:c_off + c] = False
    n = int(bad.sum())
    if n:
        first = int(np.flatnonzero(bad)[0])
        el = full.reshape(-1)[first]
        raise AssertionError("%s: %d elements outside channels [%d, %d) of %d differ from the fill 0x%02X; first at %s (holds %r)" % (
            what, n, c_off, c_off + c, ld, byte, _where(first, full.shape), el))


def assert_same_bits(a, b, what=""):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, "%s: %s %s vs %s %s" % (what, a.shape, a.dtype, b.shape, b.dtype)
    if a.size == 0:
        return
    bad = (_bits(a) != _bits(b)).any(axis=-1)
    n = int(bad.sum())
    if n:
        first = int(np.flatnonzero(bad)[0])
        shape = a.shape if a.ndim else (1,)
        raise AssertionError("%s: %d of %d elements differ in their bits; first at %s (%r vs %r)" % (
            what, n, a.size, _where(first, shape), a.reshape(-1)[first], b.reshape(-1)[first]))


def assert_finite(a, what=""):
    a = np.asarray(a)
    if a.dtype.kind == "f":
        bad = ~np.isfinite(a)
        if bad.any():
            raise AssertionError("%s: %d non-finite elements; first at %s" % (what, int(bad.sum()), _where(np.flatnonzero(bad)[0], a.shape if a.ndim else (1,))))


def checked_dest(full, c_off, c, byte, what=""):
    """the destination slice of a row buffer whose outside was pre-filled with `byte` -- after checking that the outside still holds it"""
    assert_outside_fill(full, c_off, c, byte, what)
    return np.ascontiguousarray(np.asarray(full)[..., c_off:c_off + c])


class Out:
    """one destination of a case: the whole row buffer as read back and the slice the kernel was given"""

    def __init__(self, name, full, c_off=0, c=None):
        self.name, self.full, self.c_off = name, np.asarray(full), int(c_off)
        self.c = int(self.full.shape[-1] - self.c_off if c is None else c) if self.full.ndim else 1

    @property
    def dest(self):
        return self.full[..., self.c_off:self.c_off + self.c] if self.full.ndim else self.full


# ---- completeness: which functions of the header are compute entries ------------------------------------------------------------------------
RUNTIME_GROUP = re.compile(r"^si_hip_(version|error_string|device|set_device|get_device|malloc|free|host|memset|memcpy|stream|event|ipc|"
                           r"enable_peer_access|graph)(_|$)")
EXEMPT_SUFFIXES = ("_supported", "_eligible", "_preferred", "_weight_elems", "_pack_weight_host", "_kernel_name", "_kernel_name_form",
                   "_tile_variant", "_workspace_bytes", "_host")


def header_functions(path=HEADER):
    """the si_hip_* functions the header declares, in order (comments and the inline C++ overloads' bodies do not count twice)"""
    src = open(path).read()
    src = re.sub(r"/\*.*?\*/", " ", src, flags=re.S)
    src = re.sub(r"//[^\n]*", " ", src)
    names = []
    for m in re.finditer(r"\b(si_hip_\w+)\s*\(", src):
        if m.group(1) not in names:
            names.append(m.group(1))
    return names


def is_exempt(name):
    """by RULE, never by list: the runtime group and the host-side query / packing functions"""
    return bool(RUNTIME_GROUP.match(name)) or name.endswith(EXEMPT_SUFFIXES)


def compute_entries(path=HEADER):
    return [n for n in header_functions(path) if not is_exempt(n)]


# ---- the case matrix ------------------------------------------------------------------------------------------------------------------------
def R(seed, shape, lo=-1.0, hi=1.0, dtype=np.float32):
    r = np.random.Generator(np.random.Philox(seed))
    return (lo + (hi - lo) * r.random(shape, dtype=np.float32)).astype(dtype)


def U8(seed, shape):
    return np.random.Generator(np.random.Philox(seed)).integers(0, 256, shape, dtype=np.uint8)


class Case:
    def __init__(self, cid, entries, run, plan=None, refuse=None):
        self.id, self.run, self.plan, self.refuse = cid, run, plan or {}, refuse
        self.entries = tuple("si_hip_" + e for e in ((entries,) if isinstance(entries, str) else entries))


CASES = []


def case(cid, entries, plan=None, refuse=None):
    def deco(fn):
        CASES.append(Case(cid, entries, fn, plan, refuse))
        return fn
    return deco


def _hw(v):
    return (int(v), int(v)) if np.isscalar(v) else (int(v[0]), int(v[1]))


def _conv(cid, entry, xs, oc, k=1, s=1, p=0, d=1, g=1, res=False, half=False, plan=None, seed=0, image=False, out_f32=False, **views):
    """a conv2d / conv2d_f16 case: input xs, ragged everything in `views` (in_ld, in_c_off, out_ld, out_c_off, res_ld, res_c_off)"""
    dt = np.float16 if half and not image else np.float32
    k, s, p, d = _hw(k), _hw(s), _hw(p), _hw(d)     # each an int (both axes) or an (h, w) pair
    oh = (xs[1] + 2 * p[0] - ((k[0] - 1) * d[0] + 1)) // s[0] + 1
    ow = (xs[2] + 2 * p[1] - ((k[1] - 1) * d[1] + 1)) // s[1] + 1

    def run(hops, F):
        x = R(seed + 1, xs, 0.0 if image else -1.0, 1.0, dt)
        w = R(seed + 2, (oc, xs[3] // g) + k, -0.3, 0.3)
        b = R(seed + 3, (oc,), -0.5, 0.5)
        r = R(seed + 4, (xs[0], oh, ow, oc), -1, 1, np.float16 if half else np.float32) if res else None
        kw = dict(views)
        if res:
            kw["res_fill"] = F
        fn = hops.conv2d_f16 if half else hops.conv2d
        if out_f32:
            kw["out_f32"] = True
        y = fn(x, w, b, s, p, d, g, act1="silu", residual=r, in_fill=F, out_fill=F, full=True, **kw)
        return [Out("y", y, views.get("out_c_off", 0), oc)]
    CASES.append(Case(cid, entry, run, plan))


# fp32 implicit GEMM: the fast pointwise kernel with a zero-padded K tail (ic = 24, 40, 72), dense and as the LAST slice of a concat row (the
# slice ends at the allocation's end: the K tail vector of the last pixel of the last image would be the first access behind it)
_conv("conv_pw_k24_last_slice", "conv2d_f32", (2, 9, 7, 24), 40, in_ld=56, in_c_off=32, out_ld=48, out_c_off=4)
_conv("conv_pw_k24_dense_ragged_oc13", "conv2d_f32", (2, 9, 7, 24), 13, out_ld=21, out_c_off=5)
_conv("conv_pw_k40_dense_m105", "conv2d_f32", (3, 5, 7, 40), 24)
_conv("conv_pw_k72_slices_res", "conv2d_f32", (2, 5, 7, 72), 16, res=True, in_ld=80, in_c_off=8, res_ld=32, res_c_off=16, out_ld=20, out_c_off=3)
_conv("conv_pw_k40_last_slice_unaligned_out", "conv2d_f32", (3, 5, 7, 40), 24, res=True, in_ld=52, in_c_off=12, res_ld=40, res_c_off=16,
      out_ld=29, out_c_off=5)
_conv("conv_3x3_ragged_everything", "conv2d_f32", (1, 7, 9, 5), 7, 3, 1, 1, in_ld=8, in_c_off=3, out_ld=11, out_c_off=3)
_conv("conv_3x3_s2_last_slice_res", "conv2d_f32", (2, 11, 9, 32), 48, 3, 2, 1, res=True, in_ld=64, in_c_off=32, res_ld=64, res_c_off=16,
      out_ld=64, out_c_off=16)
_conv("conv_3x3_k24_last_slice", "conv2d_f32", (3, 7, 5, 24), 36, 3, 1, 1, in_ld=32, in_c_off=8, out_ld=40, out_c_off=4)
_conv("conv_5x5_s3_m_not_tile", "conv2d_f32", (5, 13, 9, 20), 36, 5, 3, 2, in_ld=24, in_c_off=4, out_ld=39, out_c_off=3)
_conv("conv_one_pixel", "conv2d_f32", (1, 1, 1, 4), 4, in_ld=8, in_c_off=4, out_ld=8, out_c_off=4)
_conv("conv_one_channel", "conv2d_f32", (1, 3, 3, 1), 1, 3, 1, 1, in_ld=3, in_c_off=2, out_ld=3, out_c_off=1)
_conv("conv_dilated", "conv2d_f32", (1, 9, 9, 8), 8, 3, 1, 2, 2, in_ld=16, in_c_off=8, out_ld=12, out_c_off=4)
_conv("conv_grouped_s2", "conv2d_f32", (2, 9, 9, 64), 96, 3, 2, 1, g=8, in_ld=96, in_c_off=32, out_ld=100, out_c_off=4)
_conv("conv_grouped_generic", "conv2d_f32", (1, 6, 6, 48), 48, 1, 1, 0, g=6, in_ld=56, in_c_off=8, out_ld=51, out_c_off=3)
_conv("conv_depthwise_slices_res", "conv2d_f32", (2, 9, 11, 12), 12, 3, 1, 1, g=12, res=True, in_ld=20, in_c_off=8, res_ld=24, res_c_off=12,
      out_ld=24, out_c_off=12)
_conv("conv_depthwise_scalar_c10", "conv2d_f32", (2, 5, 7, 10), 10, 3, 2, 1, g=10, in_ld=13, in_c_off=3, out_ld=15, out_c_off=5)
# the stems (conv_stem_roll.hip / conv_smallc.hip): odd oh / ow, the dropped second row, ragged column tile, the image as a slice
_conv("stem_6x6_odd", "conv2d_f32", (2, 19, 21, 3), 32, 6, 2, 2, image=True, out_ld=40, out_c_off=4)
_conv("stem_6x6_image_slice", "conv2d_f32", (1, 18, 20, 3), 32, 6, 2, 2, image=True, in_ld=4, in_c_off=1, out_ld=37, out_c_off=5)
_conv("stem_7x7", "conv2d_f32", (2, 15, 17, 3), 64, 7, 2, 3, image=True, out_ld=72, out_c_off=8)
_conv("stem_3x3_oc16", "conv2d_f32", (2, 17, 13, 3), 16, 3, 2, 1, image=True, out_ld=24, out_c_off=4)
_conv("conv_forced_tile4", "conv2d_f32", (2, 11, 9, 32), 48, 3, 2, 1, plan=dict(f32_tile=4), in_ld=64, in_c_off=32, out_ld=64, out_c_off=16)
# rectangular kernels / strides / pads, one per family (values: tests/test_gpu_rect.py): the fast implicit GEMM's 1x7 strip, the zero-padded-K 1x1
# at stride (2,1), the depthwise column kernel with kh != KW, the 6x7 stem on the small-channel kernel
_conv("rect_conv_1x7_last_slice", "conv2d_f32", (1, 9, 11, 64), 64, (1, 7), 1, (0, 3), in_ld=96, in_c_off=32, out_ld=72, out_c_off=8)
_conv("rect_conv_pw_k24_s2x1_last_slice", "conv2d_f32", (2, 9, 7, 24), 40, 1, (2, 1), 0, in_ld=56, in_c_off=32, out_ld=48, out_c_off=4)
_conv("rect_depthwise_cols_3x5_s2x1_res", "conv2d_f32", (2, 9, 11, 16), 16, (3, 5), (2, 1), (1, 2), g=16, res=True, in_ld=24, in_c_off=8, res_ld=32,
      res_c_off=16, out_ld=32, out_c_off=16)
_conv("rect_stem_6x7_odd", "conv2d_f32", (2, 19, 21, 3), 32, (6, 7), 2, (2, 3), image=True, out_ld=40, out_c_off=4)


def _wino(cid, entry, xs, oc, pad=1, tile=2, plan=None, split=False, **views):
    oh, ow = xs[1] + 2 * pad - 2, xs[2] + 2 * pad - 2

    def run(hops, F):
        x, w, b = R(11, xs), R(12, (oc, xs[3], 3, 3), -0.3, 0.3), R(13, (oc,), -0.5, 0.5)
        r = R(14, (xs[0], oh, ow, oc))
        if split:
            y, flag = hops.conv2d_wino23_split(x, w, b, (pad, pad), act1="silu", residual=r, return_flag=True, in_fill=F, res_fill=F, out_fill=F,
                                               full=True, **views)
            return [Out("y", y, views.get("out_c_off", 0), oc), Out("range_flag", np.array([flag], np.uint32))]
        y = hops.conv2d_winograd(x, w, b, (pad, pad), act1="silu", residual=r, tile=tile, in_fill=F, res_fill=F, out_fill=F, full=True, **views)
        return [Out("y", y, views.get("out_c_off", 0), oc)]
    CASES.append(Case(cid, entry, run, plan))


_V16 = dict(in_ld=48, in_c_off=32, res_ld=48, res_c_off=16, out_ld=64, out_c_off=16)    # 16-byte aligned slices; the input is the row's last
_V3 = dict(in_ld=40, in_c_off=8, res_ld=37, res_c_off=5, out_ld=35, out_c_off=3)        # out / residual rows that are not 16-byte aligned
_wino("wino23_odd_13x17", "conv2d_wino23_f32", (2, 13, 17, 16), 32, **_V16)
_wino("wino23_odd_unaligned_out", "conv2d_wino23_f32", (2, 7, 5, 32), 32, **_V3)
_wino("wino23_pad0_oc96", "conv2d_wino23_f32", (1, 9, 8, 32), 96, pad=0, in_ld=64, in_c_off=32, res_ld=128, res_c_off=32, out_ld=100, out_c_off=4)
# (forced forms: wino23_form / wino23_ocg here, split3_bm and f16_slab_w2 below travel in the call's plan, and the C-ABI has no query that reports
# the form a launch took -- unlike f16_tile, which the test checks through si_hip_conv2d_f16_tile_variant -- so these cases hand the plan over
# and cannot confirm it was honoured)
_wino("wino23_form32", "conv2d_wino23_f32", (3, 7, 5, 32), 32, plan=dict(wino23_form=32), in_ld=64, in_c_off=32, res_ld=48, res_c_off=16, out_ld=64, out_c_off=16)
_wino("wino23_form16", "conv2d_wino23_f32", (3, 7, 5, 32), 32, plan=dict(wino23_form=16), in_ld=64, in_c_off=32, res_ld=48, res_c_off=16, out_ld=64, out_c_off=16)
_wino("wino23_ocg2", "conv2d_wino23_f32", (2, 5, 7, 32), 64, plan=dict(wino23_ocg=2), in_ld=64, in_c_off=32, res_ld=96, res_c_off=32, out_ld=67, out_c_off=3)
_wino("wino43_odd_13x17", "conv2d_wino43_f32", (2, 13, 17, 16), 32, tile=4, **_V16)
_wino("wino43_smaller_than_a_tile", "conv2d_wino43_f32", (2, 3, 3, 16), 32, tile=4, **_V3)
_wino("wino43_pad0_oc96", "conv2d_wino43_f32", (1, 9, 8, 32), 96, pad=0, tile=4, in_ld=64, in_c_off=32, res_ld=128, res_c_off=32, out_ld=100, out_c_off=4)
_wino("wino23_split_odd_13x17", "conv2d_wino23_split_f32", (2, 13, 17, 16), 32, split=True, **_V16)
_wino("wino23_split_unaligned_out", "conv2d_wino23_split_f32", (2, 7, 5, 32), 64, split=True, in_ld=40, in_c_off=8, res_ld=69, res_c_off=5, out_ld=67, out_c_off=3)


def _split3(cid, xs, oc, k, s, plan=None, res=True, **views):
    k, s = _hw(k), _hw(s)
    p = (k[0] // 2, k[1] // 2)
    oh, ow = (xs[1] + 2 * p[0] - k[0]) // s[0] + 1, (xs[2] + 2 * p[1] - k[1]) // s[1] + 1

    def run(hops, F):
        x, w, b = R(21, xs, -2, 2), R(22, (oc, xs[3]) + k, -0.2, 0.2), R(23, (oc,), -0.5, 0.5)
        r = R(24, (xs[0], oh, ow, oc)) if res else None
        y, flag = hops.conv2d_split3(x, w, b, s, p, act1="silu", residual=r, return_flag=True, in_fill=F, res_fill=F, out_fill=F, full=True,
                                     **views)
        return [Out("y", y, views.get("out_c_off", 0), oc), Out("range_flag", np.array([flag], np.uint32))]
    CASES.append(Case(cid, "conv2d_split3_f32", run, plan))


_split3("split3_pw_ragged_oc40_last_slice", (3, 9, 9, 160), 40, 1, 1, in_ld=192, in_c_off=32, res_ld=48, res_c_off=8, out_ld=48, out_c_off=4)
_split3("split3_3x3_s2_32ch", (2, 11, 13, 32), 64, 3, 2, in_ld=64, in_c_off=32, res_ld=96, res_c_off=32, out_ld=67, out_c_off=3)
_split3("rect_split3_1x5_last_slice", (2, 9, 11, 64), 48, (1, 5), 1, in_ld=96, in_c_off=32, res_ld=64, res_c_off=16, out_ld=52, out_c_off=4)
for _bm in (-1, 32, 64, 128):
    _split3("split3_3x3_s2_bm%d" % _bm, (2, 13, 11, 128), 96, 3, 2, plan=dict(split3_bm=_bm), in_ld=160, in_c_off=32, res_ld=128, res_c_off=32,
            out_ld=100, out_c_off=4)


def _siblings(cid, entry, fn_name, xs, oa, ob, half=False, **views):
    def run(hops, F):
        dt = np.float16 if half else np.float32
        x = R(31, xs, -1, 1, dt)
        wa, wb = R(32, (oa, xs[3], 1, 1), -0.3, 0.3), R(33, (ob, xs[3], 1, 1), -0.3, 0.3)
        ya, yb = getattr(hops, fn_name)(x, wa, R(34, (oa,)), wb, R(35, (ob,)), act1="silu", in_fill=F, out_fill=F, full=True, **views)
        return [Out("out", ya, views.get("out_c_off", 0), oa), Out("out2", yb, views.get("out2_c_off", 0), ob)]
    CASES.append(Case(cid, entry, run))


_siblings("split_siblings", "conv2d_split_f32", "conv2d_split", (2, 5, 7, 64), 32, 64, in_ld=96, in_c_off=32, out_ld=48, out_c_off=16,
          out2_ld=160, out2_c_off=96)
_siblings("split_siblings_unaligned", "conv2d_split_f32", "conv2d_split", (3, 3, 5, 40), 32, 24, in_ld=52, in_c_off=12, out_ld=35, out_c_off=3,
          out2_ld=29, out2_c_off=5)
_siblings("split3_siblings", "conv2d_split3_split_f32", "conv2d_split3_split", (3, 5, 7, 64), 32, 96, in_ld=96, in_c_off=32, out_ld=64,
          out_c_off=32, out2_ld=128, out2_c_off=32)
_siblings("split_siblings_f16", "conv2d_split_f16", "conv2d_split_f16", (2, 5, 7, 64), 32, 64, half=True, in_ld=96, in_c_off=32, out_ld=48,
          out_c_off=16, out2_ld=160, out2_c_off=96)


def _upcat(cid, entry, n, lh, lw, cl, cs, oc, scale, up_first, split_oc=0, half=False, split3=False, **views):
    def run(hops, F):
        dt = np.float16 if half else np.float32
        oh, ow = int(lh * scale[0]), int(lw * scale[1])
        low, skip = R(41, (n, lh, lw, cl), -1, 1, dt), R(42, (n, oh, ow, cs), -1, 1, dt)
        w, b = R(43, (oc, cl + cs, 1, 1), -0.3, 0.3), R(44, (oc,), -0.5, 0.5)
        kw = dict(views, in_fill=F, out_fill=F, full=True)
        if half:
            y = hops.conv2d_upcat_f16(low, skip, w, b, scale, up_first, act1="silu", split_oc=split_oc, **kw)
        else:
            y = hops.conv2d_upcat(low, skip, w, b, scale, up_first, act1="silu", split_oc=split_oc, split3=split3, **kw)
        if not split_oc:
            return [Out("out", y, views.get("out_c_off", 0), oc)]
        return [Out("out", y[0], views.get("out_c_off", 0), split_oc), Out("out2", y[1], views.get("out2_c_off", 0), oc - split_oc)]
    CASES.append(Case(cid, entry, run))


# the concat buffer as the LAST slice of a wider row, the low-resolution source as the last slice of its own, the destinations as slices at
# 16-byte aligned offsets and (where the entry stores dwords) at offsets that are not
_upcat("upcat_skip_first_ragged_m", "conv2d_upcat_f32", 3, 5, 7, 32, 96, 32, (2.0, 2.0), False, in_ld=160, in_c_off=32, low_ld=64, low_c_off=32,
       out_ld=48, out_c_off=16)
_upcat("upcat_unaligned_out", "conv2d_upcat_f32", 2, 3, 5, 32, 32, 40, (2.0, 2.0), True, in_ld=96, in_c_off=32, low_ld=36, low_c_off=4, out_ld=45, out_c_off=5)
_upcat("upcat_split_nonsquare", "conv2d_upcat_f32", 1, 4, 6, 32, 32, 96, (3.0, 2.0), True, split_oc=32, in_ld=96, in_c_off=32, low_ld=64, low_c_off=32,
       out_ld=48, out_c_off=16, out2_ld=67, out2_c_off=3)
_upcat("upcat_dense", "conv2d_upcat_f32", 3, 5, 7, 32, 96, 32, (2.0, 2.0), False)
_upcat("split3_upcat_ragged_oc", "conv2d_split3_upcat_f32", 3, 5, 7, 64, 192, 160, (2.0, 2.0), False, split3=True, in_ld=320, in_c_off=64, low_ld=96,
       low_c_off=32, out_ld=165, out_c_off=5)
_upcat("split3_upcat_split", "conv2d_split3_upcat_f32", 2, 5, 5, 128, 128, 128, (2.0, 2.0), True, split_oc=64, split3=True, in_ld=288, in_c_off=32,
       low_ld=160, low_c_off=32, out_ld=96, out_c_off=32, out2_ld=80, out2_c_off=16)
_upcat("upcat_f16_ragged_oc", "conv2d_upcat_f16", 3, 5, 7, 64, 192, 96, (2.0, 2.0), False, half=True, in_ld=320, in_c_off=64, low_ld=96, low_c_off=32,
       out_ld=101, out_c_off=5)
_upcat("upcat_f16_split_nonsquare", "conv2d_upcat_f16", 1, 4, 6, 32, 64, 64, (3.0, 2.0), True, split_oc=32, half=True, in_ld=128, in_c_off=32, low_ld=64,
       low_c_off=32, out_ld=48, out_c_off=16, out2_ld=64, out2_c_off=32)
_upcat("upcat_f16_dense", "conv2d_upcat_f16", 3, 5, 7, 64, 192, 96, (2.0, 2.0), False, half=True)


def _detect_operands(n, levels, ne, half=False, na=3):
    feats, ws, bs, grids, anchors = [], [], [], [], []
    for i, (h, c) in enumerate(levels):
        feats.append(R(50 + i, (n, h, h, c), -1, 1, np.float16 if half else np.float32))
        ws.append(R(60 + i, (na * ne, c, 1, 1), -0.3, 0.3))
        bs.append(R(70 + i, (na * ne,), -0.5, 0.5))
        gy, gx = np.meshgrid(np.arange(h, dtype=np.float32), np.arange(h, dtype=np.float32), indexing="ij")
        grids.append(np.broadcast_to(np.stack([gx - 0.5, gy - 0.5], -1)[None, None], (1, na, h, h, 2)).copy())
        anchors.append(np.broadcast_to(R(80 + i, (1, na, 1, 1, 2), 5, 300), (1, na, h, h, 2)).copy())
    return feats, ws, bs, grids, anchors, [8.0, 16.0, 32.0][:len(levels)], na


def _detect(cid, entries, n, levels, ne=85, kind="f32", plan=None, **views):
    def run(hops, F):
        ops = _detect_operands(n, levels, ne, kind == "f16")
        if kind == "split3":
            y, flags = hops.yolo_detect_split3(*ops, return_flags=True, in_fill=F, **views)
            return [Out("detect", y), Out("range_flags", np.array(flags, np.uint32))]
        if kind == "f16":
            tiles = [hops.yolo_f16_tile((n, h, h, c), 3, ne) for h, c in levels]
            return [Out("detect", hops.yolo_detect_f16(*ops, in_fill=F, **views)), Out("tile_form", np.array(tiles, np.int32))]
        return [Out("detect", hops.yolo_detect(*ops, fused=(kind == "fused"), in_fill=F, **views))]
    CASES.append(Case(cid, entries, run, plan))


# maps smaller than a row tile and batch 5: one tile spans several images and ends mid-tile
_detect("detect_conv_then_decode", ("yolo_decode_f32", "conv2d_f32"), 5, ((4, 32), (2, 64), (1, 96)))
_detect("detect_fused_epilogue", "conv2d_yolo_f32", 5, ((4, 32), (2, 64), (1, 96)), kind="fused")
_detect("detect_fused_features_last_slice", "conv2d_yolo_f32", 5, ((4, 32), (2, 64), (1, 96)), kind="fused", in_pad=32, in_c_off=32)
_detect("detect_split3_features_last_slice", "conv2d_split3_yolo_f32", 3, ((5, 128), (3, 192), (1, 64)), kind="split3", in_pad=32, in_c_off=32)
_detect("detect_split3_tile_kernel_last_slice", "conv2d_split3_yolo_f32", 2, ((9, 256), (10, 128)), ne=30, kind="split3", plan=dict(split3_bm=-1),
        in_pad=64, in_c_off=64)
_detect("detect_f16_tile_kernel_last_slice", ("conv2d_yolo_f16", "conv2d_yolo_f16_tile"), 2, ((9, 256), (3, 128), (1, 512)), kind="f16", in_pad=32,
        in_c_off=32)
_detect("detect_f16_generic_last_slice", ("conv2d_yolo_f16", "conv2d_yolo_f16_tile"), 2, ((9, 256), (5, 64)), kind="f16", plan=dict(f16_detect_tile=0),
        in_pad=8, in_c_off=8)
_detect("detect_fused_ne25", "conv2d_yolo_f32", 2, ((5, 64), (3, 32)), ne=25, kind="fused")
_detect("detect_split3", "conv2d_split3_yolo_f32", 3, ((5, 128), (3, 192), (1, 64)), kind="split3")
_detect("detect_split3_tile_kernel", "conv2d_split3_yolo_f32", 2, ((9, 256), (10, 128)), ne=30, kind="split3", plan=dict(split3_bm=-1))
_detect("detect_split3_bm32", "conv2d_split3_yolo_f32", 2, ((9, 128),), kind="split3", plan=dict(split3_bm=32))
_detect("detect_f16_tile_kernel", ("conv2d_yolo_f16", "conv2d_yolo_f16_tile"), 2, ((9, 256), (3, 128), (1, 512)), kind="f16")
_detect("detect_f16_generic_tiles", ("conv2d_yolo_f16", "conv2d_yolo_f16_tile"), 2, ((9, 256), (5, 64)), kind="f16", plan=dict(f16_detect_tile=0))
_detect("detect_f16_ne25", ("conv2d_yolo_f16", "conv2d_yolo_f16_tile"), 3, ((5, 128), (2, 32)), ne=25, kind="f16")


@case("conv_transpose_k3s2_slices", "conv_transpose2d_f32")
def _(hops, F):
    x, w, b = R(91, (2, 5, 7, 8)), R(92, (8, 6, 3, 3), -0.3, 0.3), R(93, (6,))
    y = hops.conv_transpose2d(x, w, b, (2, 2), (1, 1), (1, 1), in_ld=16, in_c_off=8, in_fill=F, out_ld=11, out_c_off=3, out_fill=F, full=True)
    return [Out("y", y, 3, 6)]


@case("conv_transpose_k2s2_odd_channels", "conv_transpose2d_f32")
def _(hops, F):
    x, w, b = R(94, (1, 5, 6, 5)), R(95, (5, 7, 2, 2), -0.3, 0.3), R(96, (7,))
    y = hops.conv_transpose2d(x, w, b, (2, 2), in_ld=8, in_c_off=3, in_fill=F, out_ld=12, out_c_off=5, out_fill=F, full=True)
    return [Out("y", y, 5, 7)]


@case("linear_ragged", "linear_f32")
def _(hops, F):
    return [Out("y", hops.linear(R(101, (3, 50)), R(102, (7, 50), -0.3, 0.3), R(103, (7,))))]


@case("linear_one_row_one_col", "linear_f32")
def _(hops, F):
    return [Out("y", hops.linear(R(104, (1, 129)), R(105, (1, 129), -0.3, 0.3), None))]


def _pixelwise(cid, entries, call, shape, dtype=np.float32, lo=-2.0, hi=2.0, **views):
    """an elementwise / pooling wrapper with the common view hooks; call(hops, x, **hooks) returns the full destination(s)"""
    def run(hops, F):
        x = R(111, shape, lo, hi, dtype)
        y = call(hops, x, in_fill=F, out_fill=F, full=True, **views)
        ys = y if isinstance(y, (list, tuple)) else [y]
        return [Out("y%d" % i, v, views.get("out_c_off", 0), shape[-1]) for i, v in enumerate(ys)]
    CASES.append(Case(cid, entries, run))


_VA = dict(in_ld=16, in_c_off=8, out_ld=24, out_c_off=12)        # vector path: 16-byte aligned slices, the input the row's last
_VH = dict(in_ld=16, in_c_off=8, out_ld=32, out_c_off=16)        # the same in halves
for _dt, _sfx, _c, _vu, _va in ((np.float32, "f32", 6, dict(in_ld=9, in_c_off=3, out_ld=11, out_c_off=5), _VA),
                                (np.float16, "f16", 12, dict(in_ld=17, in_c_off=5, out_ld=19, out_c_off=3), _VH)):
    _mp = "maxpool2d" if _sfx == "f32" else "maxpool2d_f16"
    _ap = "adaptive_avgpool2d" if _sfx == "f32" else "adaptive_avgpool2d_f16"
    _ac = "activation" if _sfx == "f32" else "activation_f16"
    _un = "unary_op" if _sfx == "f32" else "unary_op_f16"
    _pixelwise("maxpool_k3s2_" + _sfx, "maxpool2d_" + _sfx, lambda hops, x, _f=_mp, **kw: getattr(hops, _f)(x, (3, 3), (2, 2), (1, 1), **kw),
               (2, 9, 7, 8), _dt, -3, -1, **_va)
    _pixelwise("rect_maxpool_k3x2_s2x1_" + _sfx, "maxpool2d_" + _sfx, lambda hops, x, _f=_mp, **kw: getattr(hops, _f)(x, (3, 2), (2, 1), (1, 0), **kw),
               (2, 9, 7, 8), _dt, -3, -1, **_va)
    _pixelwise("maxpool_k5s1_unaligned_" + _sfx, "maxpool2d_" + _sfx, lambda hops, x, _f=_mp, **kw: getattr(hops, _f)(x, (5, 5), (1, 1), (2, 2), **kw),
               (2, 5, 7, _c), _dt, -3, -1, **_vu)
    _pixelwise("avgpool_3x4_" + _sfx, "adaptive_avgpool2d_" + _sfx, lambda hops, x, _f=_ap, **kw: getattr(hops, _f)(x, (3, 4), **kw),
               (2, 12, 8, 8), _dt, **_va)
    _pixelwise("avgpool_global_unaligned_" + _sfx, "adaptive_avgpool2d_" + _sfx, lambda hops, x, _f=_ap, **kw: getattr(hops, _f)(x, (1, 1), **kw),
               (2, 7, 7, _c), _dt, **_vu)
    _pixelwise("activation_silu_" + _sfx, "activation_" + _sfx, lambda hops, x, _f=_ac, **kw: getattr(hops, _f)("silu", x, **kw), (3, 5, 7, 8), _dt, **_va)
    _pixelwise("activation_hardswish_unaligned_" + _sfx, "activation_" + _sfx, lambda hops, x, _f=_ac, **kw: getattr(hops, _f)("hardswish", x, **kw),
               (1, 3, 5, _c), _dt, **_vu)
    _pixelwise("unary_neg_" + _sfx, "unary_" + _sfx, lambda hops, x, _f=_un, **kw: getattr(hops, _f)(1, x, **kw), (3, 5, 7, 8), _dt, **_va)
    _pixelwise("unary_abs_unaligned_one_pixel_" + _sfx, "unary_" + _sfx, lambda hops, x, _f=_un, **kw: getattr(hops, _f)(0, x, **kw), (1, 1, 1, _c), _dt, **_vu)
    # SPPF's pool chain: three destinations as slices of ONE kind of row; the large finite fill would win every max it reached
    _pixelwise("maxpool5_chain3_" + _sfx, "maxpool5_chain3_" + _sfx,
               lambda hops, x, _h=(_sfx == "f16"), **kw: hops.maxpool5_chain3(x, half=_h, out_c_off=(kw.pop("out_c_off"),) * 3, **kw),
               (3, 13, 7, 24), _dt, -3, -1, in_ld=48, in_c_off=24, out_ld=96, out_c_off=48)
_pixelwise("maxpool5_chain3_one_pixel_f32", "maxpool5_chain3_f32", lambda hops, x, **kw: hops.maxpool5_chain3(x, out_c_off=(kw.pop("out_c_off"),) * 3, **kw),
           (2, 1, 1, 4), np.float32, -3, -1, in_ld=8, in_c_off=4, out_ld=12, out_c_off=4)
_pixelwise("upsample_nearest_scale", "upsample_nearest_f32", lambda hops, x, **kw: hops.upsample_nearest(x, 1.5, 2.5, (7, 17), **kw), (1, 5, 7, 2),
           in_ld=5, in_c_off=3, out_ld=7, out_c_off=5)
_pixelwise("upsample_nearest_x2_vector", "upsample_nearest_f32", lambda hops, x, **kw: hops.upsample_nearest(x, 2.0, 2.0, **kw), (2, 3, 5, 8), **_VA)
_pixelwise("upsample_nearest_size", "upsample_nearest_steps_f32", lambda hops, x, **kw: hops.upsample_nearest_size(x, (12, 7), **kw), (2, 5, 6, 8), **_VA)
_pixelwise("upsample_nearest_size_unaligned", "upsample_nearest_steps_f32", lambda hops, x, **kw: hops.upsample_nearest_size(x, (3, 11), **kw), (1, 5, 4, 3),
           in_ld=5, in_c_off=2, out_ld=8, out_c_off=5)
_pixelwise("upsample_bilinear_f32", "upsample_bilinear_f32", lambda hops, x, **kw: hops.upsample_bilinear(x, (11, 9), **kw), (2, 5, 6, 8), **_VA)
_pixelwise("upsample_bilinear_unaligned_f32", "upsample_bilinear_f32", lambda hops, x, **kw: hops.upsample_bilinear(x, scale=2, align_corners=True, **kw),
           (1, 3, 4, 5), in_ld=8, in_c_off=3, out_ld=10, out_c_off=5)
_pixelwise("upsample_bilinear_f16", "upsample_bilinear_f16", lambda hops, x, **kw: hops.upsample_bilinear(x, (11, 9), **kw), (2, 5, 6, 8), np.float16, **_VH)
_pixelwise("upsample_bilinear_odd_offsets_f16", "upsample_bilinear_f16", lambda hops, x, **kw: hops.upsample_bilinear(x, scale=2, **kw), (1, 3, 4, 6),
           np.float16, in_ld=9, in_c_off=3, out_ld=11, out_c_off=5)
_pixelwise("copy_channels_vector", "copy_channels_f32", lambda hops, x, **kw: hops.copy_channels(x, **kw), (2, 3, 5, 12), in_ld=20, in_c_off=8, out_ld=24, out_c_off=4)
_pixelwise("copy_channels_unaligned", "copy_channels_f32", lambda hops, x, **kw: hops.copy_channels(x, **kw), (2, 3, 5, 7), in_ld=10, in_c_off=3, out_ld=12, out_c_off=5)
_pixelwise("binary_scalar_rdiv", "binary_scalar_f32", lambda hops, x, **kw: hops.binary_scalar(8, x, 3.0, **kw), (1, 3, 5, 7), np.float32, 0.5, 2.0,
           in_ld=10, in_c_off=3, out_ld=12, out_c_off=5)
_pixelwise("binary_scalar_add_vector", "binary_scalar_f32", lambda hops, x, **kw: hops.binary_scalar(0, x, 1.75, **kw), (2, 3, 5, 8), **_VA)
_pixelwise("batchnorm", "batchnorm2d_f32", lambda hops, x, **kw: hops.batchnorm2d(x, R(1, (8,)), R(2, (8,), 0.5, 2), R(3, (8,)), R(4, (8,)), 1e-5, **kw),
           (2, 3, 5, 8), **_VA)
_pixelwise("batchnorm_unaligned", "batchnorm2d_f32", lambda hops, x, **kw: hops.batchnorm2d(x, R(1, (5,)), R(2, (5,), 0.5, 2), R(3, (5,)), R(4, (5,)), 1e-5, **kw),
           (2, 3, 5, 5), in_ld=8, in_c_off=3, out_ld=10, out_c_off=5)
_pixelwise("convert_roundtrip", ("convert_f32_f16", "convert_f16_f32"), lambda hops, x, **kw: hops.convert_roundtrip_f16(x, **kw), (3, 5, 5, 8), **_VA)
_pixelwise("convert_roundtrip_unaligned", ("convert_f32_f16", "convert_f16_f32"), lambda hops, x, **kw: hops.convert_roundtrip_f16(x, **kw), (3, 5, 5, 10),
           in_ld=13, in_c_off=3, out_ld=15, out_c_off=5)
_pixelwise("binary_same_add_f16", "binary_same_f16", lambda hops, x, **kw: hops.binary_same_f16("add", x, R(112, x.shape, -2, 2, np.float16), b_ld=24, b_c_off=16, **kw),
           (2, 5, 7, 8), np.float16, **_VH)
_pixelwise("binary_bcast_mul_f16", "binary_bcast_f16", lambda hops, x, **kw: hops.binary_bcast_f16("mul", x, R(113, (3, 72), 0, 1, np.float16), **kw),
           (3, 5, 7, 72), np.float16, in_ld=80, in_c_off=8, out_ld=88, out_c_off=16)


@case("segment_labels_f32", "segment_labels_f32")
def _(hops, F):
    return [Out("labels", hops.segment_labels(R(121, (2, 5, 6, 5)), (11, 13), in_ld=8, in_c_off=3, in_fill=F))]


@case("segment_labels_f16", "segment_labels_f16")
def _(hops, F):
    return [Out("labels", hops.segment_labels(R(122, (2, 5, 6, 8), -1, 1, np.float16), (7, 9), True, in_ld=16, in_c_off=8, in_fill=F))]


@case("segment_labels_one_class_f32", "segment_labels_f32")
def _(hops, F):
    return [Out("labels", hops.segment_labels(R(123, (1, 2, 3, 1)), (5, 5), in_ld=3, in_c_off=2, in_fill=F))]


@case("cat_spatial_axes", "cat_axis_f32")
def _(hops, F):
    return [Out("h", hops.cat([R(131, (2, 3, 4, 6)), R(132, (2, 5, 4, 6))], 1)), Out("w", hops.cat([R(133, (2, 3, 4, 5)), R(134, (2, 3, 6, 5))], 2))]


@case("cat_channels", "copy_channels_f32")
def _(hops, F):
    return [Out("c", hops.cat([R(135, (2, 3, 5, 3)), R(136, (2, 3, 5, 2)), R(137, (2, 3, 5, 4))], 3))]


@case("flatten_slice", "nhwc_to_nchw_f32")
def _(hops, F):
    return [Out("y", hops.flatten_nhwc(R(141, (2, 3, 5, 6)), in_ld=9, in_c_off=3, in_fill=F))]


@case("binary_broadcasts", "binary_f32")
def _(hops, F):
    a, v = R(151, (2, 6, 5, 16), 0.5, 3), R(152, (2, 1, 1, 16), 0.5, 2)
    a6, b6 = R(153, (3, 5, 7, 6), 0.5, 2), R(154, (3, 1, 1, 6), 0.5, 2)
    k = dict(in_fill=F, out_fill=F, full=True)
    return [Out("same", hops.binary_op(1, a, R(155, a.shape), in_ld=32, in_c_off=16, b_ld=48, b_c_off=32, out_ld=48, out_c_off=16, **k), 16, 16),
            Out("x/se", hops.binary_op(3, a, v, in_ld=32, in_c_off=16, b_ld=32, b_c_off=16, out_ld=37, out_c_off=5, **k), 5, 16),
            Out("se-x", hops.binary_op(1, v, a, a.shape, in_ld=19, in_c_off=3, b_ld=32, b_c_off=16, out_ld=32, out_c_off=16, **k), 16, 16),
            Out("c6", hops.binary_op(2, a6, b6, in_ld=9, in_c_off=3, b_ld=11, b_c_off=5, out_ld=11, out_c_off=5, **k), 5, 6),
            Out("both", hops.binary_op(0, R(156, (1, 3, 1, 4)), R(157, (2, 3, 5, 1)), in_ld=8, in_c_off=4, b_ld=3, b_c_off=2, out_ld=7, out_c_off=3, **k), 3, 4)]


# ---- pre / post processing: rows that do not fill the staging blocks, max_det below the picks, zero rows ----
@case("letterbox", ("letterbox_u8_f32", "letterbox_batch_u8_f32"))
def _(hops, F):
    hr, wr, _, pt, pl = hops.letterbox_geometry(30, 50, 63, 63)
    return [Out("one", hops.letterbox(U8(161, (hr, wr, 3)), 63, 63, pt, pl)), Out("batch", hops.letterbox_batch(U8(162, (3, hr, wr, 3)), 63, 63, pt, pl))]


@case("letterbox_batch_aligned", "letterbox_batch_u8_f32")
def _(hops, F):
    hr, wr, _, pt, pl = hops.letterbox_geometry(48, 64, 64, 64)
    return [Out("batch", hops.letterbox_batch(U8(163, (2, hr, wr, 3)), 64, 64, pt, pl))]


@case("resize_u8", "resize_bilinear_u8c3")
def _(hops, F):
    return [Out("down", hops.resize_bilinear_u8c3(U8(164, (2, 33, 47, 3)), 20, 64)), Out("up_one_row", hops.resize_bilinear_u8c3(U8(165, (2, 1, 5, 3)), 3, 9)),
            Out("one_col", hops.resize_bilinear_u8c3(U8(166, (1, 7, 1, 3)), 2, 4))]


@case("resize_letterbox", "resize_letterbox_batch_u8_f32")
def _(hops, F):
    return [Out("odd", hops.resize_letterbox_batch(U8(167, (3, 31, 17, 3)), 63, 63)), Out("wide", hops.resize_letterbox_batch(U8(168, (2, 45, 60, 3)), 64, 64))]


def _post(cid, n, rows, nc, thr, max_det=None, adjust=False):
    def run(hops, F):
        from util import synthetic_predictions
        pred = synthetic_predictions(100 + rows + nc, n, rows, nc=nc, n_gt=5, hot_frac=0.3) if rows else np.zeros((n, 0, 5 + nc), np.float32)
        adj = np.array([[80, 0, 0.5925926, 810, 1080], [0, 80, 1.0, 640, 480], [10, 20, 1.7, 300, 200]] * 2, np.float32)[:n] if adjust else None
        dets, cnt = hops.yolo_postprocess(pred, thr, 0.45, False, adj, max_det=max_det)
        return [Out("counts", np.asarray(cnt, np.int32))] + [Out("image%d" % i, d) for i, d in enumerate(dets)]
    CASES.append(Case(cid, "yolo_postprocess_f32", run))


_post("postprocess_rows_1000", 5, 1000, 3, 0.10, adjust=True)
_post("postprocess_all_survive", 2, 700, 20, -1.0)
_post("postprocess_max_det_below_picks", 2, 2000, 10, 0.25, max_det=5)
_post("postprocess_zero_rows", 2, 0, 80, 0.25)
_post("postprocess_one_class_64_rows", 1, 64, 1, 0.25)


# ---- fp16 storage path ----
_conv("f16_pw_k24_last_slice", "conv2d_f16", (2, 9, 7, 24), 72, half=True, in_ld=56, in_c_off=32, out_ld=88, out_c_off=8)
_conv("f16_pw_k40_dense_m105_f32_out", "conv2d_f16", (3, 5, 7, 40), 120, half=True, out_f32=True, out_ld=125, out_c_off=5)
_conv("f16_pw_k72_slices_res", "conv2d_f16", (2, 5, 7, 72), 24, half=True, res=True, in_ld=80, in_c_off=8, res_ld=40, res_c_off=16, out_ld=40, out_c_off=8)
_conv("f16_3x3_k40_last_slice", "conv2d_f16", (3, 11, 9, 40), 72, 5, 1, 2, half=True, in_ld=64, in_c_off=24, out_ld=80, out_c_off=8)
_conv("f16_3x3_s2_k72_ragged_oc130", "conv2d_f16", (2, 11, 9, 72), 130, 3, 2, 1, half=True, res=True, in_ld=80, in_c_off=8, res_ld=136, res_c_off=3,
      out_ld=135, out_c_off=5)
_conv("f16_3x3_odd_element_offsets", "conv2d_f16", (2, 7, 5, 64), 48, 3, 1, 2, 2, half=True, res=True, res_ld=53, res_c_off=5, out_ld=51, out_c_off=3)
_conv("f16_grouped", "conv2d_f16", (2, 5, 5, 64), 64, 3, 1, 1, g=2, half=True, in_ld=96, in_c_off=32, out_ld=80, out_c_off=16)
_conv("f16_s2c32_patch_kernel", "conv2d_f16", (3, 19, 25, 32), 64, 3, 2, 1, half=True, res=True, in_ld=64, in_c_off=32, res_ld=96, res_c_off=32, out_ld=96, out_c_off=16)
_conv("f16_s2c32_generic_tiles", "conv2d_f16", (3, 19, 25, 32), 64, 3, 2, 1, half=True, res=True, plan=dict(f16_s2c32=0), in_ld=64, in_c_off=32, res_ld=96,
      res_c_off=32, out_ld=96, out_c_off=16)
_conv("f16_slab_ragged", "conv2d_f16", (2, 13, 17, 128), 128, 3, 1, 1, half=True, res=True, in_ld=160, in_c_off=32, res_ld=160, res_c_off=32, out_ld=160, out_c_off=16)
_conv("f16_slab_one_wave", "conv2d_f16", (1, 7, 9, 128), 128, 3, 1, 1, half=True, plan=dict(f16_slab_w2=0), in_ld=160, in_c_off=32, out_ld=160, out_c_off=16)
for _t in (0, 3, 7, 9, 10, 11):
    _conv("f16_tile%d" % _t, "conv2d_f16", (2, 11, 9, 64), 96, 3, 2, 1, half=True, res=True, plan=dict(f16_tile=_t), in_ld=96, in_c_off=32, res_ld=128,
          res_c_off=32, out_ld=128, out_c_off=16)
_conv("f16_depthwise_slices_res", "conv2d_depthwise_f16", (2, 7, 7, 16), 16, 3, 2, 1, g=16, half=True, res=True, in_ld=24, in_c_off=8, res_ld=32, res_c_off=16,
      out_ld=32, out_c_off=8)
_conv("f16_depthwise_5x5_c72", "conv2d_depthwise_f16", (2, 9, 7, 72), 72, 5, 1, 2, g=72, half=True, in_ld=80, in_c_off=8, out_ld=88, out_c_off=16)
_conv("f16_stem_6x6_odd", "conv2d_stem_f16", (2, 19, 21, 3), 32, 6, 2, 2, half=True, image=True, out_ld=40, out_c_off=8)
_conv("f16_stem_6x6_image_slice_odd_out", "conv2d_stem_f16", (1, 18, 20, 3), 32, 6, 2, 2, half=True, image=True, in_ld=4, in_c_off=1, out_ld=37, out_c_off=5)
_conv("f16_stem_7x7_odd_width", "conv2d_stem_f16", (1, 15, 17, 3), 64, 7, 2, 3, half=True, image=True, out_ld=96, out_c_off=32)
_conv("rect_f16_7x1_last_slice", "conv2d_f16", (1, 11, 9, 64), 64, (7, 1), 1, (3, 0), half=True, in_ld=96, in_c_off=32, out_ld=80, out_c_off=16)
_conv("rect_f16_stem_6x7_odd", "conv2d_stem_f16", (2, 19, 21, 3), 32, (6, 7), 2, (2, 3), half=True, image=True, out_ld=40, out_c_off=8)
_conv("f16_stem_3x3_oc16", "conv2d_stem_f16", (2, 17, 13, 3), 16, 3, 2, 1, half=True, image=True, out_ld=24, out_c_off=8)


@case("stem_split3", "conv2d_stem_split3_f32")
def _(hops, F):
    y, flag = hops.conv2d_stem_split3(R(171, (2, 19, 20, 3), 0, 1), R(172, (32, 3, 6, 6), -0.3, 0.3), R(173, (32,)), act1="silu", return_flag=True,
                                      out_ld=40, out_c_off=4, out_fill=F, full=True)
    return [Out("y", y, 4, 32), Out("range_flag", np.array([flag], np.uint32))]


@case("stem_split3_7x7_unaligned_out", "conv2d_stem_split3_f32")
def _(hops, F):
    y, flag = hops.conv2d_stem_split3(R(174, (1, 15, 16, 3), 0, 1), R(175, (64, 3, 7, 7), -0.3, 0.3), R(176, (64,)), (2, 2), (3, 3), act1="relu",
                                      return_flag=True, out_ld=69, out_c_off=5, out_fill=F, full=True)
    return [Out("y", y, 5, 64), Out("range_flag", np.array([flag], np.uint32))]


def _stem_ops(n, ih, iw, oc=64):
    return (R(181, (n, ih, iw, 3), 0, 1), R(182, (32, 3, 6, 6), -0.3, 0.3), R(183, (32,)), R(184, (oc, 32, 3, 3), -0.3, 0.3), R(185, (oc,)))


@case("stem_s2c32_partial_tile_oc32", "conv2d_stem_s2c32_f16")
def _(hops, F):
    return [Out("y", hops.conv_stem_s2c32_f16(*_stem_ops(1, 20, 24, 32), out_ld=48, out_c_off=16, out_fill=F, full=True), 16, 32)]


@case("stem_s2c32_ragged_tiles", "conv2d_stem_s2c32_f16")
def _(hops, F):
    return [Out("y", hops.conv_stem_s2c32_f16(*_stem_ops(2, 38, 52), out_ld=69, out_c_off=5, out_fill=F, full=True), 5, 64)]


@case("stem_s2c32_pw_split_slices", "conv2d_stem_s2c32_pw_f16")
def _(hops, F):
    ya, yb = hops.conv_stem_s2c32_pw_f16(*_stem_ops(2, 38, 52), R(186, (64, 64, 1, 1), -0.3, 0.3), R(187, (64,)), split_oc=32, out_ld=48, out_c_off=16,
                                         out2_ld=64, out2_c_off=32, out_fill=F, full=True)
    return [Out("out", ya, 16, 32), Out("out2", yb, 32, 32)]


@case("stem_s2c32_pw_whole", "conv2d_stem_s2c32_pw_f16")
def _(hops, F):
    y = hops.conv_stem_s2c32_pw_f16(*_stem_ops(1, 20, 24), R(186, (64, 64, 1, 1), -0.3, 0.3), R(187, (64,)), split_oc=0, out_ld=72, out_c_off=8, out_fill=F,
                                    full=True)
    return [Out("out", y, 8, 64)]


def _pair(cid, n, hh, ww, c, res, **views):
    def run(hops, F):
        x = R(191, (n, hh, ww, c), -1, 1, np.float16)
        y = hops.conv_pw_slab_f16(x, R(192, (c, c, 1, 1), -0.15, 0.15), R(193, (c,)), R(194, (c, c, 3, 3), -0.1, 0.1), R(195, (c,)),
                                  residual=x if res else None, in_fill=F, res_fill=F, out_fill=F, full=True, **views)
        return [Out("y", y, views.get("out_c_off", 0), c)]
    CASES.append(Case(cid, "conv2d_pw_slab_f16", run))


_pair("pair_slab_128_ragged", 2, 13, 17, 128, True, in_ld=136, in_c_off=8, res_ld=160, res_c_off=32, out_ld=160, out_c_off=16)
_pair("pair_slab_256_one_slab", 1, 7, 9, 256, False, in_ld=264, in_c_off=8, out_ld=288, out_c_off=16)
_pair("pair_patch_64", 3, 8, 16, 64, True, in_ld=72, in_c_off=8, res_ld=96, res_c_off=32, out_ld=96, out_c_off=16)
_pair("pair_patch_32", 1, 8, 16, 32, True, in_ld=40, in_c_off=8, res_ld=64, res_c_off=32, out_ld=64, out_c_off=16)


@case("c3_tail_cv3_slices", "conv2d_pw_cv3_f16")
def _(hops, F):
    c, sh = 64, (3, 8, 16, 64)
    x, z = R(201, sh, -1, 1, np.float16), R(202, sh, -1, 1, np.float16)
    y = hops.conv_pw_cv3_f16(x, R(203, (c, c, 1, 1), -0.15, 0.15), R(204, (c,)), R(205, (c, c, 3, 3), -0.1, 0.1), R(206, (c,)), z,
                             R(207, (128, 128, 1, 1), -0.15, 0.15), R(208, (128,)), residual=x, z_ld=128, z_c_off=64, z_fill=F, in_ld=72, in_c_off=8, in_fill=F,
                             res_ld=96, res_c_off=32, res_fill=F, out_ld=192, out_c_off=32, out_fill=F, full=True)
    return [Out("y", y, 32, 128)]


def entries_driven():
    return sorted({e for c in CASES for e in c.entries})
