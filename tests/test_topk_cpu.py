"""CPU: the C-ABI of include/si_topk.h without a device (names, the bound table, every refusal before a launch, the workspace of a refused
descriptor) and detect_topk_plan.h as a stand-alone C++ program under ASan and UBSan (a child process)."""
import ctypes as C
import os
import subprocess

import containment as ct
from simpleinfer_amd import _native, hipops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "si_topk.h")
BADARG, UNSUPPORTED = -1, -2
ENTRIES = ["si_hip_detect_topk_kernel_name", "si_hip_detect_topk_postprocess_f32", "si_hip_detect_topk_workspace_bytes"]


def test_header_and_bound_table(native_libs):
    H, _ = native_libs
    assert sorted(ct.header_functions(HEADER)) == sorted(H._si_topk_signatures) == ENTRIES
    raw = C.CDLL(_native.LIB_HIP_PATH)   # a handle of its own: nothing but the dynamic symbol table answers
    assert all(hasattr(raw, name) for name in ENTRIES)
    assert C.sizeof(_native.SiDetectTopkDesc) == 48 and _native.SiDetectTopkDesc.image_ld.offset == 24
    assert hipops.DETECT_TOPK_MAX_DET == 1024


def test_refusals_without_a_device(native_libs):
    """every refusal happens before any device call: the pointers are compared, never followed"""
    H, _ = native_libs
    P, A, W = C.c_void_p(1 << 40), C.c_void_p(1 << 41), C.c_void_p(1 << 42)
    outs = dict(dets=1 << 43, counts=1 << 44, src_rows=None, net_boxes=None, extras=None)
    good = dict(n=2, rows=100, classes=3, extra=2, layout="channels", max_det=50)
    desc = lambda **kw: hipops.detect_topk_desc(**{**good, **kw})
    need = hipops.detect_topk_workspace_bytes(desc())
    assert need > 0 and hipops.detect_topk_kernel_name(desc()) == "topk_hist_kernel<SI_DETECT_CHANNELS>"
    assert hipops.detect_topk_kernel_name(desc(layout="rows")) == "topk_hist_kernel<SI_DETECT_ROWS>"

    def call(d, pred=P, ws=W, ws_bytes=need, out=True, **o):
        so = _native.SiDetectPostOut(**{**outs, **o})
        return H.si_hip_detect_topk_postprocess_f32(C.byref(d) if d is not None else None, pred, A, C.byref(so) if out else None, ws, ws_bytes, None)

    assert call(None) == call(desc(), pred=None) == call(desc(), out=False) == call(desc(), ws=None) == call(desc(), counts=None) == BADARG
    assert call(desc(), dets=None) == BADARG and call(desc(), pred=C.c_void_p(P.value + 2)) == BADARG and call(desc(), ws_bytes=need - 1) == BADARG
    assert H.si_hip_detect_topk_workspace_bytes(None) == 0 and hipops.detect_topk_kernel_name(desc(), 258) == "none"
    bad = [dict(n=0), dict(rows=0), dict(rows=-1), dict(classes=0), dict(extra=-1), dict(max_det=-1), dict(layout=2), dict(box_format=2),
           dict(multi_label=2), dict(ld=99), dict(layout="rows", ld=8), dict(image_ld=9 * 100 - 1)]
    unsupported = [dict(max_det=1025), dict(n=65536), dict(rows=1 << 16, classes=1 << 15, layout="rows"), dict(rows=1 << 20, classes=2047),
                   dict(image_ld=(1 << 46) + 1)]
    for kws, rc in ((bad, BADARG), (unsupported, UNSUPPORTED)):
        for kw in kws:
            assert call(desc(**kw)) == rc and hipops.detect_topk_workspace_bytes(desc(**kw)) == 0, kw
            assert hipops.detect_topk_kernel_name(desc(**kw)) == "none", kw
    assert hipops.detect_topk_workspace_bytes(desc(max_det=0)) > 0 and hipops.detect_topk_workspace_bytes(desc(max_det=1024, n=65535)) > 0
    # O(n * (bins + chunks + max_det)): the classes do not enter, the rows only through their chunks
    assert hipops.detect_topk_workspace_bytes(desc(classes=80)) == need == hipops.detect_topk_workspace_bytes(desc(rows=256, ld=256))


def test_plan_stand_alone_under_sanitizers(tmp_path):
    exe = str(tmp_path / "test_topk_plan")
    subprocess.check_call(["g++", "-std=c++17", "-O0", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-static-libasan", "-static-libubsan", "-I" + os.path.join(ROOT, "simpleinfer_amd", "csrc", "hip"),
                           os.path.join(ROOT, "tests", "cpp", "test_topk_plan.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "topk plan ok" in r.stdout and "runtime error" not in r.stderr, r.stdout[-4000:] + r.stderr[-4000:]
